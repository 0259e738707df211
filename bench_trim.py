#!/usr/bin/env python3
"""Benchmark of the batched GPU silence trimming (b2s_hip.vocoder.trim_silence_intervals_batch) on MI355X.

    python bench_trim.py [--runs 20] [--warmup 3] [--cpu-baseline]

Two workloads of 64 utterances with the reference's trim_silence_intervals parameters (top_db 50, frame_length 6400, hop 200):
`full` = 64 x 199 800 samples (1000 mel frames of audio), and `ragged` = the vocoder benchmark's seeded lengths, 200 * (T - 1) samples
for T in 240..1000.  The signals are the silence tests' gated bursts over a noise floor (tests/silence_ref.py), resident on the device.
ms_per_batch comes from device events around the split and gather launches (workspace and output allocation included, no host
read-back), median over --runs timed calls after --warmup; ms_with_readback is the wall time of the public call, which also reads
out_lengths back.  GB/s is over the algorithmic bytes: every sample read once, wav_out [B, Lmax] written once.  --cpu-baseline times
the fp64 NumPy restatement on one utterance of each workload's mean length.  One JSON line is printed.
"""
import argparse
import json
import time

import numpy as np
import torch

from benchtime import time_calls

PEAK_HBM_GBS = 8000.0
HOP = 200


def time_wall(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ms))


def workload(name, lengths, runs, warmup, seed):
    import silence_ref as R
    from b2s_hip import vocoder
    B, Lmax = len(lengths), max(lengths)
    pad = np.zeros((B, Lmax), np.float32)
    for i, n in enumerate(lengths):
        pad[i, :n] = R.fixture_signal(n, seed + i)
    wavs = torch.from_numpy(pad).cuda()
    params = vocoder.trim_params()

    def device_only():
        return vocoder._gather_device(vocoder._split_device(wavs, lengths, *params))

    med, lo, hi = time_calls(device_only, runs, warmup)
    wall = time_wall(lambda: vocoder.trim_silence_intervals_batch(wavs, lengths), runs, warmup)
    out, out_lens = vocoder.trim_silence_intervals_batch(wavs, lengths)
    want = R.trim_silence_intervals(pad[0, :lengths[0]])
    if out_lens[0] != len(want) or not np.array_equal(out[0, :out_lens[0]].cpu().numpy(), want):
        raise RuntimeError("%s: utterance 0 differs from the restatement" % name)
    bytes_ = 4 * (sum(lengths) + B * Lmax)
    return {"B": B, "samples": int(sum(lengths)), "Lmax": Lmax, "kept_fraction": round(sum(out_lens) / float(sum(lengths)), 3),
            "ms_per_batch": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "ms_with_readback": round(wall, 4),
            "audio_s_per_s": round(sum(lengths) / 16000.0 / (med / 1e3), 1), "model_GB": round(bytes_ / 1e9, 4),
            "GBs": round(bytes_ / 1e9 / (med / 1e3), 1), "frac_hbm_8TBs": round(bytes_ / (med / 1e3) / (PEAK_HBM_GBS * 1e9), 4)}


def cpu_baseline(n):
    import silence_ref as R
    w = R.fixture_signal(n, 1)
    R.trim_silence_intervals(w)
    t = time.perf_counter()
    for _ in range(3):
        R.trim_silence_intervals(w)
    return (time.perf_counter() - t) / 3 * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-baseline", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_trim.py needs a GPU (there is no CPU path)")
    a.runs = max(a.runs, 5)
    import hyperparams
    hyperparams.hparams.override_from_dict(hyperparams.DEFAULTS)
    rng = np.random.default_rng(1234)
    ragged = [HOP * (int(x) - 1) for x in rng.integers(240, 1001, size=64)]
    res = {"bench": "trim", "device": torch.cuda.get_device_name(0), "params": list(__import__("silence_ref").TRIM_PARAMS),
           "full": workload("full", [199800] * 64, a.runs, a.warmup, 1000),
           "ragged": workload("ragged", ragged, a.runs, a.warmup, 2000)}
    if a.cpu_baseline:
        ms = cpu_baseline(199800)
        res["cpu_baseline"] = {"what": "fp64 NumPy restatement (tests/silence_ref.py), one 199 800-sample utterance on one core",
                               "ms_per_utterance": round(ms, 3),
                               "speedup_vs_full": round(ms * 64 / res["full"]["ms_per_batch"], 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
