#!/usr/bin/env python3
"""Benchmark of the batched GPU monotonic alignment search and the duration error (b2s_hip.durations) on MI355X.

    python bench_dur.py [--runs 20] [--warmup 3] [--cpu-baseline]

The input is what an eval hands on: bench_align.py's 64 utterances x 6 layers x 8 heads x 256 x 1000 go through select_alignments,
and its `maps` [64, 256, 1000] (65.5 MB, on the device) are searched.  Two workloads: `full` (every length at its maximum) and
`ragged` (bench_align.py's seeded lengths, encoder 40..256, decoder 240..1000; a decoder length below its encoder length is raised
to it, such an utterance would only be reported SHORT).  `mas` is the median of device-event-timed whole mas_batch calls (workspace
and output allocation, the kernel, the division for mono_focus), `error` that of duration_error_batch on the resulting durations
against a rotated copy of them, per byte (it reads its twelve integers per pair on the host, so it includes that wait).

The yardstick is the call that runs just before in an eval: `select_ms`, select_alignments on the full batch in the same process.
`mas_over_select` is the full workload's mas over it; the budget is 1.0 (turning durations on should at most double the alignment
stage).  Nobody had measured this kernel before, so the ratio is printed whichever way it falls.

Derived, not measured: `chain_floor_ms` = (T + 16 (waves - 1)) frames x 6 dependent vector instructions (two lane shifts, compare,
two selects, add) x 4 cycles of issue each at 2.4 GHz, the time of the longest utterance's dependent chain; `stream_floor_ms` = the
valid bytes over 64 CUs (one workgroup per utterance) x 10 bytes per cycle and CU at 2.4 GHz.  `x_floor` is mas over the larger.
--cpu-baseline times the NumPy restatement (tests/dur_ref.py) on the first utterance of either workload on one core and scales it
to the batch (labelled as such).  One JSON line.
"""
import argparse
import json
import time

import numpy as np
import torch

from benchtime import stat, time_calls
import bench_align

B, S, T = bench_align.B, bench_align.S, bench_align.T
BUDGET = 1.0
CLOCK_HZ, CHAIN_INSTR, ISSUE_CYC, BLOCK = 2.4e9, 6, 4, 16
BYTES_PER_CYC_CU = 10.0


def workload(maps, enc, dec, runs, warmup):
    from b2s_hip import durations
    enc_d = torch.tensor(enc, dtype=torch.int32, device="cuda")
    dec_d = torch.tensor(dec, dtype=torch.int32, device="cuda")
    out = durations.mas_batch(maps, enc_d, dec_d)
    if out["status"].cpu().numpy().any():
        raise RuntimeError("a benchmark utterance is not OK")
    again = durations.mas_batch(maps, enc_d, dec_d)
    if not (torch.equal(again["path"], out["path"]) and torch.equal(again["score"].view(torch.int64), out["score"].view(torch.int64))):
        raise RuntimeError("the search does not repeat its bits")
    dur = out["durations"]
    other = torch.zeros_like(dur)
    for b, n in enumerate(enc):
        other[b, :n] = torch.roll(dur[b, :n], 1)
    valid = sum(e * d * 4 for e, d in zip(enc, dec))
    waves = (max(enc) + 63) // 64
    chain = (max(dec) + BLOCK * (waves - 1)) * CHAIN_INSTR * ISSUE_CYC / CLOCK_HZ * 1e3
    stream = valid / (min(len(enc), 256) * BYTES_PER_CYC_CU * CLOCK_HZ) * 1e3
    res = {"B": len(enc), "S": int(maps.shape[1]), "T": int(maps.shape[2]), "valid_bytes": valid, "frames": int(sum(dec)),
           "mas": stat(time_calls(lambda: durations.mas_batch(maps, enc_d, dec_d), runs, warmup)),
           "error": stat(time_calls(lambda: durations.duration_error_batch(dur, other, enc_d, frame_ms=12.5), runs, warmup)),
           "mono_focus_mean": round(float(out["mono_focus"].mean()), 4),
           "chain_floor_ms": round(chain, 4), "stream_floor_ms": round(stream, 4), "floors_are_derived": True}
    res["gb_per_s"] = round(valid / res["mas"]["ms"] / 1e6, 1)
    res["x_floor"] = round(res["mas"]["ms"] / max(chain, stream), 2)
    return res, out


def cpu_baseline(maps, enc, dec, out, n_batch):
    import dur_ref as R
    host = maps[0].cpu().numpy()
    t = time.perf_counter()
    ref = R.mas(host, enc[0], dec[0])
    s = time.perf_counter() - t
    if not np.array_equal(ref["durations"], out["durations"][0].cpu().numpy()):
        raise RuntimeError("the GPU and the NumPy restatement disagree on the durations of utterance 0")
    if np.float64(ref["score"]).view(np.int64) != out["score"][0].cpu().numpy().view(np.int64):
        raise RuntimeError("the GPU and the NumPy restatement disagree on the score bits of utterance 0")
    return {"enc": enc[0], "dec": dec[0], "s_per_utterance": round(s, 4), "s_per_batch_scaled": round(s * n_batch, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-baseline", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dur.py needs a GPU (there is no CPU path)")
    a.runs = max(a.runs, 5)
    from b2s_hip import alignment
    layers = bench_align.make_layers(T)
    full_enc, full_dec = [S] * B, [T] * B
    enc_d = torch.tensor(full_enc, dtype=torch.int32, device="cuda")
    dec_d = torch.tensor(full_dec, dtype=torch.int32, device="cuda")
    select = time_calls(lambda: alignment.select_alignments(layers, enc_d, dec_d), a.runs, a.warmup)
    maps = alignment.select_alignments(layers, enc_d, dec_d)["maps"].clone()
    del layers
    torch.cuda.empty_cache()
    enc, dec = bench_align.make_lengths()
    dec = [max(d, e) for e, d in zip(enc, dec)]
    res = {"bench": "dur", "device": torch.cuda.get_device_name(0), "budget_mas_over_select": BUDGET,
           "select_ms": round(select[0], 4), "select_ms_min": round(select[1], 4), "select_ms_max": round(select[2], 4)}
    res["full"], out_full = workload(maps, full_enc, full_dec, a.runs, a.warmup)
    res["ragged"], out_ragged = workload(maps, enc, dec, a.runs, a.warmup)
    res["mas_over_select"] = round(res["full"]["mas"]["ms"] / select[0], 3)
    res["within_budget"] = res["mas_over_select"] <= BUDGET
    if a.cpu_baseline:
        res["cpu_baseline"] = {"what": "NumPy restatement of the search (tests/dur_ref.py) on utterance 0 of either workload on one core, data "
                                       "already on the host; scaled by the batch size (not measured at batch size)",
                               "full": cpu_baseline(maps, full_enc, full_dec, out_full, B),
                               "ragged": cpu_baseline(maps, enc, dec, out_ragged, B)}
        res["cpu_baseline"]["speedup_vs_full_mas"] = round(res["cpu_baseline"]["full"]["s_per_batch_scaled"] * 1e3 / res["full"]["mas"]["ms"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
