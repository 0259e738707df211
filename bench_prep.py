#!/usr/bin/env python3
"""Benchmark of the batched GPU corpus preparation (b2s_hip.prep.trim_audios_batch and abs_quantile_batch) on MI355X.

    python bench_prep.py [--runs 20] [--warmup 3] [--cpu-baseline]

Workload: 64 utterances of 1 to 20 s at 16 kHz (seeded lengths), the gated bursts over a noise floor of the test fixture generator
(tests/prep_ref.py bench_signal), resident on the device.  `trim` times b2s_voc_prep_trim (stages 1-7), `quantile` the order statistic
alone over the first split's intervals of the same batch.  ms_per_batch comes from device events around the launches (workspace and
output allocation included, no host read-back), median over --runs timed calls after --warmup; ms_with_readback is the wall time of the
public call.  GB/s is over the algorithmic bytes (DESIGN.md has the formula): with S = the samples of the batch, V = the samples of the
kept intervals, C = the cropped samples and O = B * (Lmax + 4000),
    trim     = 4 * (S + S + 3 V + C + B * Lmax + C + C + O)
             = split 1 reads S, peaks read S, three select passes read V each, scale reads C and writes the [B, Lmax] buffer,
               split 2 reads C, margins read C and write O
    quantile = 4 * 3 V
--cpu-baseline times the NumPy restatement (tests/prep_ref.py) on the batch's utterances on one core.  One JSON line is printed.
"""
import argparse
import json
import time

import numpy as np
import torch

from benchtime import time_calls

COPY_GBS = 6300.0             # the copy bandwidth the project measures its memory-bound kernels against
SR = 16000


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


def figures(ms, bytes_, B, samples):
    med, lo, hi = ms
    return {"ms_per_batch": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "utterances_per_s": round(B / (med / 1e3), 1),
            "audio_s_per_s": round(samples / float(SR) / (med / 1e3), 1), "model_GB": round(bytes_ / 1e9, 4),
            "GBs": round(bytes_ / 1e9 / (med / 1e3), 1), "floor_ms_at_6300GBs": round(bytes_ / (COPY_GBS * 1e9) * 1e3, 4),
            "x_floor": round(med / (bytes_ / (COPY_GBS * 1e9) * 1e3), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-baseline", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_prep.py needs a GPU (there is no CPU path)")
    a.runs = max(a.runs, 5)
    import prep_ref as P
    from b2s_hip import prep, vocoder
    rng = np.random.default_rng(4321)
    lengths = [int(x) for x in rng.integers(1 * SR, 20 * SR + 1, size=64)]
    B, Lmax = len(lengths), max(lengths)
    ws = [P.bench_signal(n, 3000 + i) for i, n in enumerate(lengths)]
    pad = np.zeros((B, Lmax), np.float32)
    for i, w in enumerate(ws):
        pad[i, :len(w)] = w
    wavs = torch.from_numpy(pad).cuda()
    gap = 16000

    # the quantities of the byte model, and a correctness check of two utterances, from one untimed call
    out, out_lens, status, n_removed, v95 = prep.trim_audios_batch(wavs, lengths, gap)
    ivs = vocoder.split_batch(wavs, lengths, *P.SPLIT1)
    for i in (0, B - 1):
        st, nr, v, o = P.trim_audio(ws[i], gap)
        same = status[i] == st and n_removed[i] == nr and (o is None or (out_lens[i] == len(o) and np.array_equal(out[i, :len(o)].cpu().numpy(), o)))
        if not same:
            raise RuntimeError("utterance %d differs from the restatement" % i)
    S_ = sum(lengths)
    kept = [P.select_intervals(w, iv)[0] for w, iv in zip(ws, ivs)]
    V = sum(e - s for k in kept for s, e in k)
    C = sum(k[-1][1] - k[0][0] for k, st in zip(kept, status) if st in (P.OK, P.LENGTH))
    O = B * (Lmax + 4000)
    trim_bytes = 4 * (S_ + S_ + 3 * V + C + B * Lmax + C + C + O)
    q_full = [np.asarray(iv) for iv in ivs]
    Vq = sum(int((iv[:, 1] - iv[:, 0]).sum()) for iv in q_full)

    trim = figures(time_calls(lambda: prep._trim_device(wavs, lengths, gap), a.runs, a.warmup), trim_bytes, B, S_)
    trim["ms_with_readback"] = round(time_wall(lambda: prep.trim_audios_batch(wavs, lengths, gap), a.runs, a.warmup), 4)
    trim["status_counts"] = [int((status == s).sum()) for s in range(4)]

    # the order statistic alone: device-resident interval lists, no read-back inside the timed call
    lib = vocoder.load()
    from b2s_hip.lib import ptr
    NI = max(len(iv) for iv in q_full)
    ivp = np.zeros((B, NI, 2), np.int32)
    for b, iv in enumerate(q_full):
        ivp[b, :len(iv)] = iv
    iv_dev, n_dev = torch.from_numpy(ivp).cuda(), torch.tensor([len(iv) for iv in q_full], dtype=torch.int32).cuda()
    lens_dev = torch.tensor(lengths, dtype=torch.int32).cuda()
    ws_q = torch.empty(lib.b2s_voc_prep_ws_bytes(B, Lmax, prep.WS_QUANTILE), dtype=torch.uint8, device="cuda")
    q_out = torch.empty(B, dtype=torch.float32, device="cuda")

    def quantile():
        vocoder.check(lib.b2s_voc_prep_abs_quantile(ptr(wavs), ptr(lens_dev), B, Lmax, ptr(iv_dev), ptr(n_dev), NI, 0.95, ptr(q_out),
                                                    ptr(ws_q), ws_q.numel(), torch.cuda.current_stream().cuda_stream))

    quant = figures(time_calls(quantile, a.runs, a.warmup), 4 * 3 * Vq, B, S_)
    want = np.array([P.abs_quantile(w, iv, 0.95) for w, iv in zip(ws, q_full)], np.float32)
    if not np.array_equal(q_out.cpu().numpy().view(np.uint32), want.view(np.uint32)):
        raise RuntimeError("abs_quantile differs from np.sort")

    res = {"bench": "prep", "device": torch.cuda.get_device_name(0), "B": B, "samples": S_, "Lmax": Lmax, "gap_threshold": gap,
           "voiced_samples": V, "cropped_samples": C, "trim": trim, "quantile": quant}
    if a.cpu_baseline:
        t = time.perf_counter()
        for w in ws:
            P.trim_audio(w, gap)
        ms = (time.perf_counter() - t) * 1e3
        res["cpu_baseline"] = {"what": "NumPy restatement (tests/prep_ref.py) of the same 64 utterances on one core", "ms_per_batch": round(ms, 1),
                               "speedup": round(ms / trim["ms_per_batch"], 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
