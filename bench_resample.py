#!/usr/bin/env python3
"""Benchmark of the batched GPU down-mix and resampling to 16 kHz (b2s_hip.prep.resample_batch) on MI355X.

    python bench_resample.py [--runs 20] [--warmup 3] [--cpu-baseline]

Workloads, all resident on the device (uniform noise of amplitude 0.5, seeded lengths):
    mono_22050     64 utterances of 1 to 20 s at 22 050 Hz, mono
    stereo_44100   the same durations at 44 100 Hz, two channels (down-mix + resampling)
    ragged_48000   64 utterances at 48 000 Hz whose durations are spread log-uniformly over 0.2 to 20 s
ms_per_call comes from device events around one b2s_voc_resample call (table kernel, down-mix, resampling; workspace and output
allocation included, no host read-back), median over --runs timed calls after --warmup.  taps is the exact number of filter taps the
batch needs (per output the two wing counts of the algorithm, edges included).  Yardsticks:
    lds_floor_ms   3 LDS dword reads per tap (two table entries, one sample) at 256 B/clk/CU x 256 CUs x 2.4 GHz.  Derived, not
                   measured; dword reads are served at 128 B/clk/CU on this chip, so a loop of dword reads cannot go under 2 x this.
    copy_ms        a device-to-device copy that moves as many bytes as the call's input plus output (measured here)
--cpu-baseline times the NumPy restatement (tests/resample_ref.py) on 1.5 s of audio per rate on one core.  One JSON line is printed.
"""
import argparse
import json
import time

import numpy as np
import torch

from benchtime import time_calls

LDS_BYTES_PER_S = 256.0 * 256 * 2.4e9         # 256 B/clk/CU, 256 CUs, 2.4 GHz
SR = 16000


def tap_count(n, orig_sr):
    """Taps of one utterance of n samples: the sum over its outputs of both wing counts."""
    import resample_ref as R
    win, delta, step, scale, ratio = R.filter_table(orig_sr)
    t = np.arange(R.lengths(n, orig_sr)[0])
    time_ = t * (1.0 / ratio)
    pos = time_.astype(np.int64)
    frac = scale * (time_ - pos)
    left = np.minimum(pos + 1, (R.NWIN - (frac * 512).astype(np.int64)) // step)
    right = np.minimum(n - pos - 1, (R.NWIN - ((scale - frac) * 512).astype(np.int64)) // step)
    return int(left.sum() + right.sum())


def workload(name, orig_sr, channels, lengths, runs, warmup, rng):
    import resample_ref as R
    from b2s_hip import prep
    B, Lmax = len(lengths), max(lengths)
    shape = (B, Lmax) if channels == 1 else (B, Lmax, channels)
    wavs = torch.zeros(shape, dtype=torch.float32, device="cuda")
    rows = {}
    order = np.argsort(lengths)
    for b, n in enumerate(lengths):
        x = rng.uniform(-0.5, 0.5, (n,) + shape[2:]).astype(np.float32)
        wavs[b, :n] = torch.from_numpy(x).cuda()
        if b in order[:2]:
            rows[b] = x
    out, n_out = prep.resample_batch(wavs, lengths, orig_sr)
    got = out.cpu().numpy()
    worst = 0.0
    for b, x in rows.items():                                    # the two shortest utterances against the restatement
        ref = R.load(x, orig_sr)
        err = float(np.abs(got[b, :len(ref)] - ref).max())
        bound = 4.0 * float(np.abs(R.load(x, orig_sr, fp32=True) - ref).max())
        if n_out[b] != len(ref) or err > bound:
            raise RuntimeError("%s: utterance %d differs from the restatement by %g (bound %g)" % (name, b, err, bound))
        worst = max(worst, err)
    med, lo, hi = time_calls(lambda: prep._resample_device(wavs, lengths, orig_sr), runs, warmup)
    taps = sum(tap_count(n, orig_sr) for n in lengths)
    outputs = int(sum(prep.resample_lengths(n, orig_sr)[0] for n in lengths))
    moved = 4 * (B * Lmax * channels + out.numel())
    src = torch.empty(moved // 8, dtype=torch.float32, device="cuda")
    dst = torch.empty_like(src)
    copy_ms = time_calls(lambda: dst.copy_(src), runs, warmup)[0]
    floor_ms = taps * 12 / LDS_BYTES_PER_S * 1e3
    tile, span = prep.resample_tile(orig_sr)
    return {"orig_sr": orig_sr, "channels": channels, "B": B, "Lmax_in": Lmax, "Lmax_out": int(out.shape[1]), "input_s": round(sum(lengths) / orig_sr, 1),
            "outputs": outputs, "taps": taps, "taps_per_output": round(taps / max(1, outputs), 1), "tile": tile, "span": span,
            "ms_per_call": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "utterances_per_s": round(B / (med / 1e3), 1),
            "audio_s_per_s": round(sum(lengths) / orig_sr / (med / 1e3), 1), "Gtaps_per_s": round(taps / 1e9 / (med / 1e3), 1),
            "lds_floor_ms": round(floor_ms, 4), "x_lds_floor": round(med / floor_ms, 2), "moved_GB": round(moved / 1e9, 4),
            "copy_ms": round(copy_ms, 4), "x_copy": round(med / copy_ms, 2), "max_err_two_shortest": worst}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-baseline", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample.py needs a GPU (there is no CPU path)")
    a.runs = max(a.runs, 5)
    rng = np.random.default_rng(4321)
    seconds = rng.uniform(1.0, 20.0, size=64)
    ragged = np.exp(rng.uniform(np.log(0.2), np.log(20.0), size=64))
    res = {"bench": "resample", "device": torch.cuda.get_device_name(0)}
    for name, sr, ch, secs in (("mono_22050", 22050, 1, seconds), ("stereo_44100", 44100, 2, seconds), ("ragged_48000", 48000, 1, ragged)):
        res[name] = workload(name, sr, ch, [int(s * sr) for s in secs], a.runs, a.warmup, rng)
        torch.cuda.empty_cache()
    if a.cpu_baseline:
        import resample_ref as R
        base = {"what": "NumPy restatement (tests/resample_ref.py, fp64) of 1.5 s of audio on one core"}
        for sr in (22050, 44100, 48000):
            x = rng.uniform(-0.5, 0.5, int(1.5 * sr)).astype(np.float32)
            t = time.perf_counter()
            R.resample(x, sr)
            base["s_per_1.5s_at_%d" % sr] = round(time.perf_counter() - t, 4)
        res["cpu_baseline"] = base
    print(json.dumps(res))


if __name__ == "__main__":
    main()
