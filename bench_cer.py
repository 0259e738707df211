#!/usr/bin/env python3
"""Benchmark of the GPU edit distance behind the CER (b2s_hip.cer, b2s_met_edit_distance) on MI355X.

    python bench_cer.py [--runs 20] [--warmup 3] [--cpu-baseline]

Three seeded workloads over int32 symbols: `eval_set` (4096 pairs, truth lengths 60..300 over a 40-symbol alphabet, the prediction
is the truth with about 10 % random edits: a whole eval set of transcriptions in one launch), `batch64` (64 such pairs: one eval
batch) and `long` (64 pairs of 4096 x 4096 over a 32-symbol alphabet: the kernel's limit on both sides).  For each: ms_per_call =
the median of device-event-timed whole edit_distance_batch calls with the breakdown (output allocation, the launch, the status
check and its copy to the host; inputs packed on the device beforehand), `gcells_per_s` over the cells sum(la * lb) of the DP
matrices, and `x_valu_floor` = ms_per_call over the VALU floor

    cells x 5 instructions per cell / (256 CUs x 4 SIMDs x 32 lanes per clock x 2.4 GHz = 78.6e12 lane-instructions per second)

(compare, select, two adds, one three-way minimum per cell; the per-step shifts and the idle lanes of the systolic fill and drain
are not in the floor, so the ratio shows them).  --cpu-baseline times the NumPy restatement of the contract (tests/edit_ref.py, one
row per NumPy call) on the first 64 pairs of `eval_set` on one core and scales it to the 4096 (labelled as such), after checking
that it agrees with the GPU on those pairs.  Nobody had measured this kernel before, so there is no pass / fail figure.  One JSON
line is printed.
"""
import argparse
import json
import time

import numpy as np
import torch

from benchtime import time_calls

INSTR_PER_CELL = 5
LANE_RATE = 256 * 4 * 32 * 2.4e9


def edited_pairs(n, seed, lo=60, hi=300, alphabet=40, rate=0.1):
    import edit_ref as R
    rng = np.random.default_rng(seed)
    truths = [rng.integers(alphabet, size=int(rng.integers(lo, hi + 1))).astype(np.int32) for _ in range(n)]
    return truths, [R.mutate(rng, t, rate, alphabet) for t in truths]


def long_pairs(n, seed, length=4096, alphabet=32):
    rng = np.random.default_rng(seed)
    return ([rng.integers(alphabet, size=length).astype(np.int32) for _ in range(n)],
            [rng.integers(alphabet, size=length).astype(np.int32) for _ in range(n)])


def workload(truths, preds, runs, warmup):
    from b2s_hip import cer
    a, b = cer.pack(truths), cer.pack(preds)
    cells = sum(x * y for x, y in zip(a.lengths, b.lengths))
    med, lo, hi = time_calls(lambda: cer.edit_distance_batch(a, b, return_ops=True), runs, warmup)
    floor_ms = cells * INSTR_PER_CELL / LANE_RATE * 1e3
    dist, ops = cer.edit_distance_batch(a, b, return_ops=True)
    return {"pairs": len(a), "max_truth": a.max_len, "max_pred": b.max_len, "cells": cells,
            "ms_per_call": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
            "gcells_per_s": round(cells / med / 1e6, 2), "valu_floor_ms": round(floor_ms, 5),
            "x_valu_floor": round(med / floor_ms, 1), "sum_dist": int(dist.sum()), "sum_ops": ops.sum(0).tolist()}, dist


def cpu_baseline(truths, preds, dist, n=64):
    import edit_ref as R
    t = time.perf_counter()
    ref = [R.edit_packed(a, b)[0] for a, b in zip(truths[:n], preds[:n])]
    s = time.perf_counter() - t
    if ref != dist[:n].cpu().tolist():
        raise RuntimeError("the GPU and the NumPy restatement disagree on the first %d pairs of eval_set" % n)
    return {"what": "NumPy restatement of the contract (one row of the DP matrix per NumPy call, packed int64 cells) on the first %d "
                    "pairs of eval_set on one core, data already on the host; scaled by %d / %d (not measured at batch size)"
                    % (n, len(truths), n), "s_measured": round(s, 3), "s_per_eval_set_scaled": round(s * len(truths) / n, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-baseline", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cer.py needs a GPU (there is no CPU path)")
    a.runs = max(a.runs, 5)
    from b2s_hip import cer
    res = {"bench": "cer", "device": torch.cuda.get_device_name(0), "max_len": cer.max_len(), "instr_per_cell": INSTR_PER_CELL,
           "lane_instr_per_s": LANE_RATE}
    truths, preds = edited_pairs(4096, 1234)
    res["eval_set"], dist = workload(truths, preds, a.runs, a.warmup)
    if a.cpu_baseline:
        res["cpu_baseline"] = cpu_baseline(truths, preds, dist)
        res["cpu_baseline"]["speedup_vs_eval_set"] = round(res["cpu_baseline"]["s_per_eval_set_scaled"] * 1e3
                                                           / res["eval_set"]["ms_per_call"])
    res["batch64"], _ = workload(*edited_pairs(64, 4321), a.runs, a.warmup)
    res["long"], _ = workload(*long_pairs(64, 99), a.runs, a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
