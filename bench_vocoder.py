#!/usr/bin/env python3
"""Benchmark of the batched GPU Griffin-Lim vocoder and mel front end (b2s_hip.vocoder) on MI355X.

    python bench_vocoder.py [--runs 10] [--warmup 2] [--n-iter 60] [--cpu-baseline]

Two workloads, 64 utterances each: `full` = 64 x 1000 frames, and `ragged` = seeded lengths in 240..1000 (the eval driver's
frame range).  ms_per_batch comes from device events around whole mel2wav_batch calls (upload of the mels excluded, workspace
allocation included), median over --runs timed calls after --warmup; wav2mel_ms the same for wav2mel_batch on the batch's
waveforms.  The byte / FLOP model (vocoder section) is computed from the shapes.  --cpu-baseline times the fp64 NumPy
restatement of the reference (tests/audio_ref.py) on ONE 1000-frame utterance and scales it to the batch (labelled as such).
One JSON line is printed.
"""
import argparse
import json
import time

import numpy as np
import torch

from benchtime import time_calls

PEAK_FP32_TFLOPS = 157.3
PEAK_HBM_GBS = 8000.0
NBIN, WIN, HOP = 1025, 800, 200


def model(frames, n_iter):
    """Bytes and FLOPs the algorithm needs for `frames` packed frames (DESIGN.md vocoder section).
    Per frame-iteration: S_t read (4.1 KB), neighbour segments (3.2 KB unique), new segment written (3.2 KB);
    two 1024-point complex FFTs (5 N log2 N each) + split / projection / windowing (~12 flop per bin and sample)."""
    fft = 2 * 5 * 1024 * 10
    per_iter_flops = fft + 12 * NBIN + 40 * WIN
    per_iter_bytes = 4 * NBIN + 4 * WIN + 4 * WIN
    flops = frames * (n_iter * per_iter_flops + fft // 2 + 2 * 80 * NBIN)
    bytes_ = frames * (n_iter * per_iter_bytes + 4 * 80 + 2 * 4 * NBIN + 2 * 4 * WIN + 4 * HOP)
    return bytes_, flops


def workload(name, lengths, n_iter, runs, warmup, seed):
    from b2s_hip import vocoder
    B, Tmax = len(lengths), max(lengths)
    g = torch.Generator(device="cuda").manual_seed(seed)
    mels = (torch.rand(B, Tmax, 80, device="cuda", generator=g) * 6.0 - 4.0).contiguous()
    out = {}
    med, lo, hi = time_calls(lambda: vocoder.mel2wav_batch(mels, lengths, n_iter=n_iter), runs, warmup)
    frames = int(sum(lengths))
    audio_s = sum(HOP * (t - 1) for t in lengths) / 16000.0
    bytes_, flops = model(frames, n_iter)
    out.update(B=B, frames=frames, n_iter=n_iter, ms_per_batch=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
               frames_per_s=round(frames / (med / 1e3)), audio_s_per_s=round(audio_s / (med / 1e3), 1),
               model_GB=round(bytes_ / 1e9, 2), model_TFLOP=round(flops / 1e12, 3),
               frac_hbm_8TBs=round(bytes_ / (med / 1e3) / (PEAK_HBM_GBS * 1e9), 3),
               frac_fp32_peak=round(flops / (med / 1e3) / (PEAK_FP32_TFLOPS * 1e12), 3))
    wav, wl = vocoder.mel2wav_batch(mels, lengths, n_iter=n_iter)
    torch.cuda.synchronize()
    if not bool(torch.isfinite(wav).all()):
        raise RuntimeError("%s: non-finite waveform" % name)
    wmed, _, _ = time_calls(lambda: vocoder.wav2mel_batch(wav, wl), runs, warmup)
    out["wav2mel_ms"] = round(wmed, 3)
    return out


def cpu_baseline(n_iter, frames_per_batch):
    import audio_ref as A
    rng = np.random.default_rng(0)
    mel = (rng.random((1000, 80)) * 6 - 4).astype(np.float32)
    t = time.perf_counter()
    A.mel2wav(mel, n_iter=n_iter)
    s = time.perf_counter() - t
    return {"what": "fp64 NumPy restatement, one 1000-frame utterance on one core, scaled to the batch (not measured at batch size)",
            "s_one_utterance": round(s, 3), "s_per_batch_scaled": round(s * frames_per_batch / 1000.0, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n-iter", type=int, default=60)
    ap.add_argument("--cpu-baseline", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vocoder.py needs a GPU (there is no CPU path)")
    a.runs = max(a.runs, 5)
    import hyperparams
    hyperparams.hparams.override_from_dict(hyperparams.DEFAULTS)
    rng = np.random.default_rng(1234)
    ragged = [int(x) for x in rng.integers(240, 1001, size=64)]
    res = {"bench": "vocoder", "device": torch.cuda.get_device_name(0), "target_ms_full": 15.0,
           "full": workload("full", [1000] * 64, a.n_iter, a.runs, a.warmup, 7),
           "ragged": workload("ragged", ragged, a.n_iter, a.runs, a.warmup, 8)}
    if a.cpu_baseline:
        res["cpu_baseline"] = cpu_baseline(a.n_iter, res["full"]["frames"])
        res["cpu_baseline"]["speedup_vs_full"] = round(res["cpu_baseline"]["s_per_batch_scaled"] * 1e3 / res["full"]["ms_per_batch"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
