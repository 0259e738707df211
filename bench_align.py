#!/usr/bin/env python3
"""Benchmark of the GPU alignment-head selection (b2s_hip.alignment, b2s_met_align_select) on MI355X.

    python bench_align.py [--runs 20] [--warmup 3] [--cpu-baseline]

The eval driver's largest job: 64 utterances, 6 decoder layers x 8 heads, S = 256 encoder positions, T = 1000 generated frames
(3.1 GB of fp32 alignments, seeded softmax maps with a distinct sharpness per head).  Three workloads: `full` (every length at its
maximum), `ragged` (seeded lengths, encoder 40..256, decoder 240..1000: what a padded batch looks like) and `ragged_odd_T` (the
same lengths with T = 999, which takes the dword-load layout).  For each: ms_per_call = the median of device-event-timed whole
select_alignments calls (workspace and output allocation, both kernels and the few tensor ops that derive layer / head / focus;
inputs already on the device), `gb_per_s` over the bytes the contract requires the reduction to read (valid rows and frames of
every head, 4 bytes each -- not the padded size), and `x_copy` = ms_per_call over the time of a device-to-device copy of that many
bytes measured in the same process (the copy reads AND writes them, so a pure reader can land below 1).  `scores_only` is the call
without maps (no slab copy).  --cpu-baseline times the NumPy restatement (tests/align_ref.py) on the first utterance of the ragged
batch and scales it to the batch (labelled as such).  Nobody had measured this kernel before, so there is no pass / fail figure.
One JSON line is printed.
"""
import argparse
import json
import time

import numpy as np
import torch

from benchtime import time_calls

B, L, H, S, T = 64, 6, 8, 256, 1000


def make_lengths(seed=1234):
    rng = np.random.default_rng(seed)
    return [int(v) for v in rng.integers(40, S + 1, size=B)], [int(v) for v in rng.integers(240, T + 1, size=B)]


def make_layers(t, seed=1234):
    """L device tensors [B, H, S, t]: softmax over s of seeded normal logits, sharpness 0.3..3.3 spread over the 48 heads."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    sharp = torch.linspace(0.3, 3.3, L * H, device="cuda").roll(L * H // 2 + 1).reshape(L, 1, H, 1, 1)
    return [torch.softmax(torch.randn(B, H, S, t, device="cuda", generator=g) * sharp[l], dim=2).contiguous() for l in range(L)]


def required_bytes(enc, dec, t):
    return sum(L * H * min(e, S) * min(d, t) * 4 for e, d in zip(enc, dec))


def copy_ms(nbytes, runs, warmup):
    src = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    return time_calls(lambda: dst.copy_(src), runs, warmup)[0]


def workload(layers, enc, dec, runs, warmup):
    from b2s_hip import alignment
    t = int(layers[0].shape[3])
    enc_d = torch.tensor(enc, dtype=torch.int32, device="cuda")
    dec_d = torch.tensor(dec, dtype=torch.int32, device="cuda")
    nbytes = required_bytes(enc, dec, t)
    med, lo, hi = time_calls(lambda: alignment.select_alignments(layers, enc_d, dec_d), runs, warmup)
    med_s, _, _ = time_calls(lambda: alignment.select_alignments(layers, enc_d, dec_d, want_maps=False), runs, warmup)
    cp = copy_ms(nbytes, runs, warmup)
    out = alignment.select_alignments(layers, enc_d, dec_d)
    return {"T": t, "required_read_bytes": nbytes, "padded_bytes": L * B * H * S * t * 4, "map_bytes_out": B * S * t * 4,
            "ms_per_call": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
            "gb_per_s": round(nbytes / med / 1e6, 1), "scores_only_ms": round(med_s, 3),
            "scores_only_gb_per_s": round(nbytes / med_s / 1e6, 1), "copy_same_bytes_ms": round(cp, 3),
            "x_copy": round(med / cp, 2), "scores_only_x_copy": round(med_s / cp, 2),
            "heads_chosen": sorted(set((out["layer"] * H + out["head"]).cpu().tolist()))}, out


def cpu_baseline(layers, enc, dec, out):
    import align_ref as R
    host = [a[:1].cpu().numpy() for a in layers]
    t = time.perf_counter()
    ref = R.select(host, enc[:1], dec[:1])
    s = time.perf_counter() - t
    if int(ref["best"][0]) != int(out["layer"][0]) * H + int(out["head"][0]):
        raise RuntimeError("the GPU and the NumPy restatement chose different heads for utterance 0")
    if abs(float(out["scores"][0].max()) - float(ref["scores"][0].max())) > 1e-9:
        raise RuntimeError("the GPU and the NumPy restatement disagree on the best score of utterance 0")
    return {"what": "NumPy restatement of the contract (vectorised max / sum / argmax, fp64 sum) on utterance 0 of the ragged batch "
                    "(enc %d, dec %d) on one core, data already on the host; scaled by the batch size (not measured at batch size)"
                    % (enc[0], dec[0]), "s_per_utterance": round(s, 4), "s_per_batch_scaled": round(s * B, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-baseline", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_align.py needs a GPU (there is no CPU path)")
    a.runs = max(a.runs, 5)
    from b2s_hip import alignment
    enc, dec = make_lengths()
    res = {"bench": "align", "device": torch.cuda.get_device_name(0), "B": B, "layers": L, "heads": H, "S": S, "T": T,
           "chunk_frames": alignment.chunk()}
    layers = make_layers(T)
    res["full"], _ = workload(layers, [S] * B, [T] * B, a.runs, a.warmup)
    res["ragged"], out = workload(layers, enc, dec, a.runs, a.warmup)
    if a.cpu_baseline:
        res["cpu_baseline"] = cpu_baseline(layers, enc, dec, out)
        res["cpu_baseline"]["speedup_vs_ragged"] = round(res["cpu_baseline"]["s_per_batch_scaled"] * 1e3 / res["ragged"]["ms_per_call"])
    del layers, out
    torch.cuda.empty_cache()
    layers = make_layers(T - 1)
    res["ragged_odd_T"], _ = workload(layers, enc, [min(d, T - 1) for d in dec], a.runs, a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
