#!/usr/bin/env python3
"""Benchmark of the batched GPU mel-cepstral distortion after DTW (b2s_hip.mcd) on MI355X.

    python bench_mcd.py [--runs 20] [--warmup 3] [--cpu-baseline]

bench_dtw.py's batch: 64 pairs with seeded ragged lengths (predictions 240..1100 frames, targets 240..1000), 80 mels, about 10 % of
the frames on each side unvoiced; order 13.  `mcd_dtw_r1` / `mcd_dtw_exact` = whole mcd_dtw_batch calls at radius 1 and with the exact
dtw (upload excluded; packing, the cepstral kernels of both sides, the host read of the voiced offsets, the DTW, the score and the
status read included), `mse_dtw_r1` = metrics.mse_dtw_batch on the same batch in the same process, `ratio_r1` the first over the
last (the gate is 1.25).  `new_kernels` times the two new steps alone with device events: cepstra_packed for both sides on packed
device rows (three launches each) and score_packed on the radius-1 paths (output allocation included), and gives their share of
the radius-1 call.  ms figures are medians of device-event-timed calls after --warmup calls.  --cpu-baseline times the NumPy restatement (tests/mcd_ref.py) on the
first 3 pairs on one core and scales it to the batch (labelled as such).  One JSON line is printed.
"""
import argparse
import json
import time

import numpy as np
import torch

from benchtime import stat, time_calls

from bench_dtw import make_batch

ORDER = 13
KEY = ("ms_per_batch", 3)            # this benchmark's name and digits for stat's median


def cpu_baseline(preds, pl, targets, tl, n=3):
    import mcd_ref as R
    t = time.perf_counter()
    R.calculate_mcd_dtw(preds[:n], pl[:n], targets[:n], tl[:n], order=ORDER, radius=1)
    s = time.perf_counter() - t
    return {"what": "NumPy restatement (voiced frames, cepstra, pure Python fastdtw radius 1, score), first %d pairs on one core, "
                    "scaled to the batch (not measured at batch size)" % n,
            "s_per_pair": round(s / n, 3), "s_per_batch_scaled": round(s / n * len(pl), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-baseline", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mcd.py needs a GPU (there is no CPU path)")
    a.runs = max(a.runs, 5)
    from b2s_hip import mcd, metrics
    preds, pl, targets, tl = make_batch()
    dp, dt = torch.from_numpy(preds).cuda(), torch.from_numpy(targets).cuda()
    res = {"bench": "mcd", "device": torch.cuda.get_device_name(0), "B": len(pl), "n_mels": int(preds.shape[2]), "order": ORDER,
           "frames_x": int(sum(pl)), "frames_y": int(sum(tl)), "gate_ratio_r1": 1.25}

    res["mcd_dtw_r1"] = stat(time_calls(lambda: mcd.mcd_dtw_batch(dp, pl, dt, tl, order=ORDER, radius=1), a.runs, a.warmup), *KEY)
    m = mcd.mcd_dtw_batch(dp, pl, dt, tl, order=ORDER, radius=1).cpu().numpy()
    if not np.all(np.isfinite(m)):
        raise RuntimeError("non-finite MCD in the benchmark batch")
    res["mcd_dtw_r1"]["mean_mcd_db"] = round(float(m.mean()), 6)
    res["mse_dtw_r1"] = stat(time_calls(lambda: metrics.mse_dtw_batch(dp, pl, dt, tl, radius=1), a.runs, a.warmup), *KEY)
    res["ratio_r1"] = round(res["mcd_dtw_r1"]["ms_per_batch"] / res["mse_dtw_r1"]["ms_per_batch"], 3)
    res["mcd_dtw_exact"] = stat(time_calls(lambda: mcd.mcd_dtw_batch(dp, pl, dt, tl, order=ORDER, radius=None),
                                           max(5, a.runs // 4), 1), *KEY)
    res["dtw_exact"] = stat(time_calls(lambda: metrics.dtw_batch(dp, pl, dt, tl, radius=None), max(5, a.runs // 4), 1), *KEY)

    # the two new steps alone, on device-resident packed rows
    xr, xo, mx = mcd.pack_batch(dp, pl)
    yr, yo, my = mcd.pack_batch(dt, tl)
    cep = time_calls(lambda: (mcd.cepstra_packed(xr, xo, mx, ORDER), mcd.cepstra_packed(yr, yo, my, ORDER)), a.runs, a.warmup)
    d = mcd.mcd_dtw_details(dp, pl, dt, tl, order=ORDER, radius=1)
    scored = {}

    def score():
        scored["mcd"] = mcd.score_packed(d["cep_x"], d["offsets_x"], d["cep_x"].shape[0], d["cep_y"], d["offsets_y"], d["cep_y"].shape[0],
                                         d["path"], d["path_offsets_device"], d["path_len"], d["dtw_status"])[0]
    sc = time_calls(score, a.runs, a.warmup)
    if not torch.equal(scored["mcd"], d["mcd"]):
        raise RuntimeError("the score kernel alone does not repeat the call's bits")
    res["new_kernels"] = {"cepstra_both_sides_ms": round(cep[0], 4), "score_ms": round(sc[0], 4),
                          "voiced_x": int(d["voiced_x"].sum()), "voiced_y": int(d["voiced_y"].sum()),
                          "path_steps": int(d["path_len"].sum()),
                          "share_of_r1_call": round((cep[0] + sc[0]) / res["mcd_dtw_r1"]["ms_per_batch"], 3)}
    if a.cpu_baseline:
        res["cpu_baseline"] = cpu_baseline(preds, pl, targets, tl)
        res["cpu_baseline"]["speedup_vs_r1"] = round(res["cpu_baseline"]["s_per_batch_scaled"] * 1e3 / res["mcd_dtw_r1"]["ms_per_batch"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
