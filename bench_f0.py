#!/usr/bin/env python3
"""Benchmark of the batched GPU YIN pitch tracker and the F0 score (b2s_hip.f0) on MI355X.

    python bench_f0.py [--runs 20] [--warmup 3] [--cpu-baseline]

Two workloads of 64 utterances: `full` = 64 x 199 800 samples (1000 frames each at hop 200), `ragged` = seeded lengths of 240..1000
frames (bench_vocoder.py's).  The audio is a harmonic tone with a wandering pitch, unvoiced stretches of noise and pauses.  The three
calls are timed apart with device events on device-resident data (output allocation included, upload excluded): `quantize_ms`
(quantize_batch on the fp32 waveforms), `yin_ms` (yin_batch on the int16 PCM, default parameters: win 800, 267 lags) and `score_ms`
(score_packed of the batch against a second take of it along the diagonal path).  ms figures are medians after --warmup calls.

`floor_ms` is derived, not measured: frames x win x (tau_max + 1) multiply-adds at the VALU fp64 FMA rate of the data sheet (78.6
TFLOP/s vector fp64 = 39.3 T FMA/s); nobody has measured that rate on these machines.  `x_floor` is yin_ms over it.
`vocoder_ms` is mel2wav_batch on 64 x 1000 frames at hp.n_iter in the same process and `yin_over_vocoder` the full workload's
yin_ms over it; the budget is 0.25 (the re-scoring vocodes both sides and has to stay dominated by that).  --cpu-baseline times
the NumPy restatement (tests/f0_ref.py) on 50 frames on one core and scales it to the batch (labelled as such).  One JSON line.
"""
import argparse
import json
import time

import numpy as np
import torch

from benchtime import stat, time_calls

SR, HOP, WIN = 16000, 200, 800
FP64_FMA_PER_S = 78.6e12 / 2
BUDGET = 0.25


def speechlike(lengths, seed):
    """[B, Lmax] fp32: per utterance a tone with 5 harmonics and a pitch that wanders in 80..300 Hz, switched every 0.2 .. 0.6 s
    between voiced, noise and a pause."""
    rng = np.random.default_rng(seed)
    out = np.zeros((len(lengths), max(lengths)), np.float32)
    for b, L in enumerate(lengths):
        f = np.clip(160.0 + np.cumsum(rng.standard_normal(L)) * 0.05, 80.0, 300.0)
        ph = 2 * np.pi * np.cumsum(f) / SR
        w = sum(np.sin(k * ph) / k for k in range(1, 6)) + 0.02 * rng.standard_normal(L)
        pos = 0
        while pos < L:
            n = int(rng.integers(SR // 5, 3 * SR // 5))
            kind = rng.integers(0, 4)
            if kind == 2:
                w[pos:pos + n] = 0.1 * rng.standard_normal(len(w[pos:pos + n]))
            elif kind == 3:
                w[pos:pos + n] *= 0.001
            pos += n
        out[b, :L] = 0.5 * w
    return out


def workload(lengths, runs, warmup, seed):
    from b2s_hip import f0
    wav = torch.from_numpy(speechlike(lengths, seed)).cuda()
    take2 = torch.from_numpy(speechlike(lengths, seed + 100)).cuda()
    q = f0.quantize_batch(wav, lengths)
    pcm = q["pcm"]
    x = f0.yin_batch(pcm, lengths)
    y = f0.yin_batch(f0.quantize_batch(take2, lengths)["pcm"], lengths)
    if x["status"].cpu().numpy().any():
        raise RuntimeError("a benchmark utterance FAILED")
    frames = x["frames"]
    prm = x["params"]
    out = {"B": len(lengths), "samples": int(sum(lengths)), "frames": int(sum(frames)), "win": prm["win"],
           "lags": prm["tau_max"] + 1, "voiced_fraction": round(float((x["tau"] > 0).double().mean()), 3)}
    out["quantize"] = stat(time_calls(lambda: f0.quantize_batch(wav, lengths), runs, warmup))
    out["yin"] = stat(time_calls(lambda: f0.yin_batch(pcm, lengths), runs, warmup))
    again = f0.yin_batch(pcm, lengths)
    if not (torch.equal(again["f0"], x["f0"]) and torch.equal(again["tau"], x["tau"])):
        raise RuntimeError("the YIN call does not repeat its bits")
    dev = pcm.device
    kept = torch.cat([torch.arange(n, dtype=torch.int32) for n in frames]).to(dev)
    koff = x["frame_offsets_device"]
    path = torch.stack([kept, kept], dim=1).contiguous()
    plen = torch.tensor(frames, dtype=torch.int32, device=dev)
    dstat = torch.zeros(len(frames), dtype=torch.int32, device=dev)
    out["score"] = stat(time_calls(lambda: f0.score_packed(x, y, kept, koff, kept, koff, path, koff, plen, dstat), runs, warmup))
    macs = out["frames"] * prm["win"] * (prm["tau_max"] + 1)
    out["gmac"] = round(macs / 1e9, 2)
    out["floor_ms"] = round(macs / FP64_FMA_PER_S * 1e3, 4)
    out["x_floor"] = round(out["yin"]["ms"] / out["floor_ms"], 2)
    return out


def cpu_baseline(frames_per_batch, n=50):
    import f0_ref as R
    pcm = R.quantize(speechlike([HOP * n], 3)[0])[0]
    t = time.perf_counter()
    R.yin(pcm[:HOP * (n - 1)], floor=R.min_energy(WIN, -40))
    s = time.perf_counter() - t
    return {"what": "NumPy restatement of YIN (tests/f0_ref.py), %d frames on one core, scaled to the full batch (not measured at "
                    "batch size)" % n, "s_per_frame": round(s / n, 5), "s_per_batch_scaled": round(s / n * frames_per_batch, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-baseline", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_f0.py needs a GPU (there is no CPU path)")
    a.runs = max(a.runs, 5)
    import hyperparams
    hp = hyperparams.hparams
    hp.override_from_dict(hyperparams.DEFAULTS)
    from b2s_hip import vocoder
    rng = np.random.default_rng(1234)
    ragged = [HOP * (int(t) - 1) for t in rng.integers(240, 1001, size=64)]
    res = {"bench": "f0", "device": torch.cuda.get_device_name(0), "fp64_fma_per_s_assumed": FP64_FMA_PER_S,
           "fp64_rate_measured_here": False, "budget_yin_over_vocoder": BUDGET,
           "full": workload([HOP * 999] * 64, a.runs, a.warmup, 7), "ragged": workload(ragged, a.runs, a.warmup, 8)}
    g = torch.Generator(device="cuda").manual_seed(7)
    mels = (torch.rand(64, 1000, 80, device="cuda", generator=g) * 6.0 - 4.0).contiguous()
    n_iter = int(hp.n_iter)
    voc = time_calls(lambda: vocoder.mel2wav_batch(mels, [1000] * 64, n_iter=n_iter), max(5, a.runs // 2), 2)
    res["vocoder_ms"] = round(voc[0], 3)
    res["vocoder_n_iter"] = n_iter
    res["yin_over_vocoder"] = round(res["full"]["yin"]["ms"] / voc[0], 4)
    res["within_budget"] = res["yin_over_vocoder"] <= BUDGET
    if a.cpu_baseline:
        res["cpu_baseline"] = cpu_baseline(res["full"]["frames"])
        res["cpu_baseline"]["speedup_vs_full_yin"] = round(res["cpu_baseline"]["s_per_batch_scaled"] * 1e3 / res["full"]["yin"]["ms"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
