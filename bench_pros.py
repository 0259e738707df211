#!/usr/bin/env python3
"""Benchmark of the batched GPU prosody targets (b2s_hip.prosody: window energy, Viterbi pitch track, unit sums) on MI355X.

    python bench_pros.py [--runs 20] [--warmup 3] [--cpu-baseline]

Two workloads of 64 utterances, bench_f0.py's: `full` = 64 x 199 800 samples (1000 frames each at hop 200) and `ragged` = its seeded
lengths of 240..1000 frames, the same speech-like audio.  Everything is timed with device events on device-resident data (output
and workspace allocation included, upload excluded), medians after --warmup calls: `energy` (energy_batch on the int16 PCM), `track`
(track_batch on the YIN result with its 137 MB CMND matrix, default parameters: 235 lags, W = 8), `units` (unit_prosody over 128
positions per utterance whose seeded durations sum to its frames) and `chain`, the three in a row.  `track_nowalk` is the same call
on a copy of the CMND matrix whose last frame holds a NaN in every utterance: the whole search runs, the utterance is FAILED and the
walk back and the refinement are skipped, so track - track_nowalk is what those two cost.

The yardstick is the call in front: `yin_cmnd`, f0.yin_batch(return_cmnd=True) on the same PCM in the same process, which produces
the matrix.  `chain_over_yin` is the full workload's chain over it; the budget is 1.0 (asking for prosody targets should at most
double the pitch stage).  Nobody had measured these kernels before, so the ratio is printed whichever way it falls.

Derived, not measured, for `track`: `stream_floor_ms` = the CMND bytes over min(B, 256) CUs (one workgroup per utterance) x 10 bytes
per cycle and CU at 2.4 GHz; `chain_floor_ms` = the longest utterance's frames x (2 W + 1) band candidates x 4 vector instructions
(add, compare, two selects) x 4 cycles of issue each at 2.4 GHz (the guide's figure for one wave's fp32 stream; fp64 is not listed
and cannot be cheaper).  `x_floor` is track over the larger.  --cpu-baseline times the NumPy restatement (tests/pros_ref.py) of the
search on utterance 0 of the full workload on one core, checks its bits against the GPU's and scales it to the batch (labelled as
such).  One JSON line.
"""
import argparse
import json
import time

import numpy as np
import torch

from benchtime import stat, time_calls
import bench_f0

B, S = 64, 128
BUDGET = 1.0
CLOCK_HZ, BAND_INSTR, ISSUE_CYC = 2.4e9, 4, 4
BYTES_PER_CYC_CU = 10.0


def workload(lengths, runs, warmup, seed):
    from b2s_hip import f0, prosody
    import dur_ref
    wav = torch.from_numpy(bench_f0.speechlike(lengths, seed)).cuda()
    pcm = f0.quantize_batch(wav, lengths)["pcm"]
    del wav
    yin_t = time_calls(lambda: f0.yin_batch(pcm, lengths, return_cmnd=True), runs, warmup)
    y = f0.yin_batch(pcm, lengths, return_cmnd=True)
    if y["status"].cpu().numpy().any():
        raise RuntimeError("a benchmark utterance FAILED")
    prm, frames = y["params"], y["frames"]
    en = prosody.energy_batch(pcm, lengths, win=prm["win"], hop=prm["hop"])
    tr = prosody.track_batch(y, en)
    again = prosody.track_batch(y, en)
    if tr["status"].cpu().numpy().any():
        raise RuntimeError("a benchmark track is not OK")
    if not (torch.equal(again["tau"], tr["tau"]) and torch.equal(again["score"].view(torch.int64), tr["score"].view(torch.int64))):
        raise RuntimeError("the search does not repeat its bits")
    rng = np.random.default_rng(seed)
    d = torch.from_numpy(np.stack([dur_ref.random_durations(rng, S, f) for f in frames]).astype(np.int32)).cuda()
    n_in = torch.full((len(frames),), S, dtype=torch.int32, device="cuda")
    un = prosody.unit_prosody(tr, en, d, n_in)
    if not set(un["status"].cpu().tolist()) <= {prosody.OK}:
        raise RuntimeError("a benchmark utterance has no unit sums")

    def chain():
        e = prosody.energy_batch(pcm, lengths, win=prm["win"], hop=prm["hop"])
        t = prosody.track_batch(y, e)
        return prosody.unit_prosody(t, e, d, n_in)
    W = tr["params"]["W"]
    cm_bytes = int(y["cmnd"].numel()) * 8
    chain_floor = max(frames) * (2 * W + 1) * BAND_INSTR * ISSUE_CYC / CLOCK_HZ * 1e3
    stream_floor = cm_bytes / (min(len(frames), 256) * BYTES_PER_CYC_CU * CLOCK_HZ) * 1e3
    res = {"B": len(frames), "samples": int(sum(lengths)), "frames": int(sum(frames)), "lags": prm["tau_max"] - prm["tau_min"] + 1,
           "W": W, "units_per_utterance": S, "cmnd_bytes": cm_bytes,
           "voiced_fraction_yin": round(float((y["tau"] > 0).double().mean()), 3),
           "voiced_fraction_track": round(float((tr["tau"] > 0).double().mean()), 3),
           "yin_cmnd": stat(yin_t),
           "energy": stat(time_calls(lambda: prosody.energy_batch(pcm, lengths, win=prm["win"], hop=prm["hop"]), runs, warmup)),
           "track": stat(time_calls(lambda: prosody.track_batch(y, en), runs, warmup)),
           "units": stat(time_calls(lambda: prosody.unit_prosody(tr, en, d, n_in), runs, warmup)),
           "chain": stat(time_calls(chain, runs, warmup)),
           "chain_floor_ms": round(chain_floor, 4), "stream_floor_ms": round(stream_floor, 4), "floors_are_derived": True}
    nan = dict(y, cmnd=y["cmnd"].clone())
    last = y["frame_offsets_device"][1:].to(torch.int64) - 1
    nan["cmnd"][last, prm["tau_max"]] = float("nan")
    res["track_nowalk"] = stat(time_calls(lambda: prosody.track_batch(nan, en), max(5, runs // 2), 2))
    del nan
    res["walk_and_refine_ms"] = round(res["track"]["ms"] - res["track_nowalk"]["ms"], 4)
    res["x_floor"] = round(res["track"]["ms"] / max(chain_floor, stream_floor), 2)
    res["chain_over_yin"] = round(res["chain"]["ms"] / res["yin_cmnd"]["ms"], 3)
    return res, y, en, tr


def cpu_baseline(y, en, tr, n_batch):
    import pros_ref as R
    prm = y["params"]
    lo, hi = int(y["frame_offsets"][0]), int(y["frame_offsets"][1])
    cm, e = y["cmnd"][lo:hi].cpu().numpy(), en["energy"][lo:hi].cpu().numpy()
    t = time.perf_counter()
    ref = R.track(cm, e, tr["params"]["floor"], prm["tau_min"], prm["tau_max"], sr=prm["sr"],
                  **{k: tr["params"][k] for k in ("u", "v", "lam", "mu", "W")})
    s = time.perf_counter() - t
    if not np.array_equal(ref["tau"], tr["tau"][lo:hi].cpu().numpy()):
        raise RuntimeError("the GPU and the NumPy restatement disagree on the track of utterance 0")
    if not np.array_equal(ref["f0"].view(np.int64), tr["f0"][lo:hi].cpu().numpy().view(np.int64)):
        raise RuntimeError("the GPU and the NumPy restatement disagree on the F0 bits of utterance 0")
    if np.float64(ref["score"]).view(np.int64) != tr["score"][0].cpu().numpy().view(np.int64):
        raise RuntimeError("the GPU and the NumPy restatement disagree on the score bits of utterance 0")
    return {"what": "NumPy restatement of the search (tests/pros_ref.py, with its tie count) on utterance 0 of the full workload on one "
                    "core, data already on the host; scaled by the batch size (not measured at batch size)",
            "frames": hi - lo, "s_per_utterance": round(s, 4), "s_per_batch_scaled": round(s * n_batch, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-baseline", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pros.py needs a GPU (there is no CPU path)")
    a.runs = max(a.runs, 5)
    import hyperparams
    hyperparams.hparams.override_from_dict(hyperparams.DEFAULTS)
    rng = np.random.default_rng(1234)
    ragged = [bench_f0.HOP * (int(t) - 1) for t in rng.integers(240, 1001, size=B)]
    res = {"bench": "pros", "device": torch.cuda.get_device_name(0), "budget_chain_over_yin": BUDGET}
    res["full"], y, en, tr = workload([bench_f0.HOP * 999] * B, a.runs, a.warmup, 7)
    if a.cpu_baseline:
        res["cpu_baseline"] = cpu_baseline(y, en, tr, B)
        res["cpu_baseline"]["speedup_vs_full_track"] = round(res["cpu_baseline"]["s_per_batch_scaled"] * 1e3 / res["full"]["track"]["ms"])
    del y, en, tr
    torch.cuda.empty_cache()
    res["ragged"] = workload(ragged, a.runs, a.warmup, 8)[0]
    res["chain_over_yin"] = res["full"]["chain_over_yin"]
    res["within_budget"] = res["chain_over_yin"] <= BUDGET
    print(json.dumps(res))


if __name__ == "__main__":
    main()
