#!/usr/bin/env python3
"""Benchmark of the batched GPU FastDTW / MSE-after-DTW metric (b2s_hip.metrics) on MI355X.

    python bench_dtw.py [--runs 20] [--warmup 3] [--cpu-baseline]

One batch of 64 pairs with seeded ragged lengths (the eval driver's ranges: predictions 240..1100 frames, targets 240..1000),
80 mel features; the targets are time-warped, noisy copies of the predictions, and about 10 % of the frames on each side are
unvoiced.  Two workloads on that batch: `mse_dtw_r1` = mse_dtw_batch at radius 1 (the eval metric: voiced compaction, fastdtw,
MSE), and `exact` = dtw_batch with radius=None (the full-matrix dtw).  ms_per_batch is the median of device-event-timed whole calls
(upload excluded; packing, workspace allocation and the kernel included) after --warmup calls.  --cpu-baseline times the pure
Python / NumPy restatement of fastdtw 0.3.4 (tests/dtw_ref.py) on the first 3 pairs and scales it to the batch (labelled as such).
One JSON line is printed.
"""
import argparse
import json
import time

import numpy as np
import torch

from benchtime import time_calls


def make_batch(B=64, dim=80, seed=1234):
    rng = np.random.default_rng(seed)
    pl = [int(v) for v in rng.integers(240, 1101, size=B)]
    tl = [int(v) for v in rng.integers(240, 1001, size=B)]
    preds = np.zeros((B, max(pl), dim), np.float32)
    targets = np.zeros((B, max(tl), dim), np.float32)
    for b in range(B):
        a = np.clip(np.cumsum(rng.standard_normal((pl[b], dim)) * 0.3, axis=0), -4, 4)
        t = np.sort(rng.uniform(0, pl[b] - 1, size=tl[b]))
        c = np.clip(a[np.round(t).astype(int)] + 0.1 * rng.standard_normal((tl[b], dim)), -4, 4)
        a[rng.random(pl[b]) < 0.1] = -4.0
        c[rng.random(tl[b]) < 0.1] = -4.0
        preds[b, :pl[b]] = a
        targets[b, :tl[b]] = c
    return preds, pl, targets, tl


def cpu_baseline(preds, pl, targets, tl, n=3):
    import dtw_ref as R
    t = time.perf_counter()
    R.calculate_mse_dtw(preds[:n], pl[:n], targets[:n], tl[:n])
    s = time.perf_counter() - t
    B = len(pl)
    return {"what": "pure Python / NumPy restatement of fastdtw 0.3.4 (radius 1) + calculate_mse_dtw, first %d pairs on one core, "
                    "scaled to the batch (not measured at batch size)" % n,
            "s_per_pair": round(s / n, 3), "s_per_batch_scaled": round(s / n * B, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-baseline", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dtw.py needs a GPU (there is no CPU path)")
    a.runs = max(a.runs, 5)
    from b2s_hip import metrics
    preds, pl, targets, tl = make_batch()
    dp, dt = torch.from_numpy(preds).cuda(), torch.from_numpy(targets).cuda()
    res = {"bench": "dtw", "device": torch.cuda.get_device_name(0), "B": len(pl), "dim": int(preds.shape[2]),
           "frames_x": int(sum(pl)), "frames_y": int(sum(tl)), "target_ms_r1": 2.0}
    med, lo, hi = time_calls(lambda: metrics.mse_dtw_batch(dp, pl, dt, tl, radius=1), a.runs, a.warmup)
    m = metrics.mse_dtw_batch(dp, pl, dt, tl, radius=1).cpu().numpy()
    if not np.all(np.isfinite(m)):
        raise RuntimeError("non-finite MSE in the benchmark batch")
    res["mse_dtw_r1"] = {"ms_per_batch": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                         "mean_mse": round(float(m.mean()), 6)}
    med, lo, hi = time_calls(lambda: metrics.dtw_batch(dp, pl, dt, tl, radius=None), max(5, a.runs // 4), 1)
    res["exact"] = {"ms_per_batch": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3)}
    if a.cpu_baseline:
        res["cpu_baseline"] = cpu_baseline(preds, pl, targets, tl)
        res["cpu_baseline"]["speedup_vs_r1"] = round(res["cpu_baseline"]["s_per_batch_scaled"] * 1e3 / res["mse_dtw_r1"]["ms_per_batch"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
