#!/usr/bin/env python3
"""Benchmark of the variance adaptor (b2s_hip.variance: embed + expand, and the transposed operation) on MI355X.

    python bench_va.py [--runs 20] [--warmup 3] [--cpu-baseline]

Two workloads of 64 utterances with D = 768 columns (the width of the memory the teacher's decoder attends over), 256 bins per
table and S = 128 positions: `full` = 128 positions and 1000 frames each, `ragged` = bench_f0.py's seeded 240..1000 frames with
seeded input lengths of 40..128; the durations are dur_ref.random_durations.  Pitch and energy bins are uniform over the 256 bins,
and once `skewed`: 40 % of the positions in pitch bin 0 (the unvoiced units of real data share one bin).

Timed are the library's whole calls on device-resident inputs with outputs and workspace allocated beforehand: `forward`
(b2s_va_forward with unit_of_frame, without h), `backward` (b2s_va_backward with both table gradients) and `pair`, one after the
other.  The yardstick is measured in the same process: `copy` = copy_ of a [total_frames, D] fp32 tensor, which reads and writes
total_frames x D x 4 bytes; forward writes as much and reads about S / T of it, backward reads as much and writes about S / T of it
plus its partial sums.  Every timed interval holds REP calls back to back (the copy's too) and is divided by REP, so that the host's
launch cost, a tenth of such a call, is paid once per interval by all of them alike.  The budget is 1.0x the copy for each direction
on its own.  Nobody had measured these kernels before, so the ratios are printed whichever way they fall.

Derived, not measured: `floor_ms` = the bytes a call must move (forward: x, the frames and unit_of_frame; backward: dy, dx, and per
table the partial-sum rows written and read back, dx read once more and the table) over the 6.3 TB/s the project takes as the
streaming rate.  --cpu-baseline times the NumPy restatement (tests/va_ref.py) of forward and backward on utterance 0 of the full
workload on one core, checks its bits against the GPU's and scales it to the batch (labelled as such).  One JSON line.
"""
import argparse
import json
import time

import numpy as np
import torch

from benchtime import stat, time_calls

B, S, D, N_BINS = 64, 128, 768, 256
BUDGET = 1.0
STREAM_BYTES_PER_S = 6.3e12
REP = 8
SKEW = 0.4


def make(frames, in_lens, seed):
    """Host arrays of one workload."""
    import dur_ref
    rng = np.random.default_rng(seed)
    dur = np.zeros((B, S), np.int32)
    for b in range(B):
        dur[b, :in_lens[b]] = dur_ref.random_durations(rng, in_lens[b], frames[b])
    off = np.concatenate(([0], np.cumsum(frames))).astype(np.int32)
    pb = rng.integers(0, N_BINS, size=(B, S)).astype(np.int32)
    skew = np.where(rng.random((B, S)) < SKEW, 0, pb).astype(np.int32)
    return {"dur": dur, "n": np.asarray(in_lens, np.int32), "off": off, "total": int(off[-1]), "pb": pb, "pb_skewed": skew,
            "eb": rng.integers(0, N_BINS, size=(B, S)).astype(np.int32), "x": rng.standard_normal((B, S, D)).astype(np.float32),
            "pt": rng.standard_normal((N_BINS, D)).astype(np.float32), "et": rng.standard_normal((N_BINS, D)).astype(np.float32)}


class Calls(object):
    """The two C calls on preallocated device tensors."""

    def __init__(self, w, batch=None):
        from b2s_hip import variance
        self.v, self.lib = variance, variance.load()
        sl = slice(None) if batch is None else slice(batch, batch + 1)
        lo, hi = (0, w["total"]) if batch is None else (int(w["off"][batch]), int(w["off"][batch + 1]))
        self.nb, self.total = (B if batch is None else 1), hi - lo
        self.t = {k: torch.from_numpy(np.ascontiguousarray(w[k][sl])).cuda() for k in ("dur", "n", "pb", "pb_skewed", "eb", "x")}
        self.t["off"] = torch.from_numpy(w["off"] if batch is None else (w["off"][batch:batch + 2] - lo).astype(np.int32)).cuda()
        self.t["pt"], self.t["et"] = torch.from_numpy(w["pt"]).cuda(), torch.from_numpy(w["et"]).cuda()
        gen = torch.Generator(device="cuda").manual_seed(5)
        self.t["dy"] = torch.randn(self.total, D, device="cuda", generator=gen)
        self.y = torch.empty(self.total, D, device="cuda")
        self.uof = torch.empty(self.total, dtype=torch.int32, device="cuda")
        self.status = torch.empty(self.nb, dtype=torch.int32, device="cuda")
        self.dx = torch.empty(self.nb, S, D, device="cuda")
        self.dpt, self.det = torch.empty(N_BINS, D, device="cuda"), torch.empty(N_BINS, D, device="cuda")
        self.ws_bytes = self.lib.b2s_va_ws_bytes(self.nb, S, D, N_BINS)
        self.ws = variance.workspace(self.ws_bytes, "cuda")

    def forward(self, pb="pb"):
        t = self.t
        self.v.check(self.lib.b2s_va_forward(t["x"].data_ptr(), t[pb].data_ptr(), t["eb"].data_ptr(), t["pt"].data_ptr(), t["et"].data_ptr(),
                                             N_BINS, t["dur"].data_ptr(), t["n"].data_ptr(), t["off"].data_ptr(), self.total, self.nb, S, D,
                                             None, self.y.data_ptr(), self.uof.data_ptr(), self.status.data_ptr(), None))

    def backward(self, pb="pb"):
        t = self.t
        self.v.check(self.lib.b2s_va_backward(t["dy"].data_ptr(), t[pb].data_ptr(), t["eb"].data_ptr(), N_BINS, t["dur"].data_ptr(),
                                              t["n"].data_ptr(), t["off"].data_ptr(), self.total, self.nb, S, D, self.dx.data_ptr(),
                                              self.dpt.data_ptr(), self.det.data_ptr(), self.status.data_ptr(), self.ws.data_ptr(),
                                              self.ws_bytes, None))

    def all_ok(self):
        return not self.status.cpu().numpy().any()


def per_call(fn, runs, warmup):
    def rep():
        for _ in range(REP):
            fn()
    med, lo, hi = time_calls(rep, runs, warmup)
    return stat((med / REP, lo / REP, hi / REP))


def first_positions(w, key):
    """How many (utterance, bin) pairs are used: the partial-sum rows of one table."""
    return int(sum(len(np.unique(w[key][b, :w["n"][b]])) for b in range(B)))


def workload(frames, in_lens, runs, warmup, seed):
    w = make(frames, in_lens, seed)
    c = Calls(w)
    c.forward()
    if not c.all_ok():
        raise RuntimeError("a benchmark utterance is not OK in forward")
    c.backward()
    if not c.all_ok():
        raise RuntimeError("a benchmark utterance is not OK in backward")
    first = [t.clone() for t in (c.y, c.dx, c.dpt, c.det)]
    c.forward(), c.backward()
    if not all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, (c.y, c.dx, c.dpt, c.det))):
        raise RuntimeError("the calls do not repeat their bits")
    total = c.total
    src, dst = torch.randn(total, D, device="cuda"), torch.empty(total, D, device="cuda")
    row = D * 4
    positions = int(w["n"].sum())
    fwd_bytes = positions * row + total * row + total * 4
    res = {"B": B, "S": S, "D": D, "n_bins": N_BINS, "positions": positions, "frames": total, "frame_bytes": total * row,
           "workspace_bytes": c.ws_bytes, "copy": per_call(lambda: dst.copy_(src), runs, warmup),
           "forward": per_call(c.forward, runs, warmup), "backward": per_call(c.backward, runs, warmup),
           "pair": per_call(lambda: (c.forward(), c.backward()), runs, warmup),
           "forward_skewed": per_call(lambda: c.forward("pb_skewed"), runs, warmup),
           "backward_skewed": per_call(lambda: c.backward("pb_skewed"), runs, warmup), "floors_are_derived": True}
    for name, key in (("backward", "pb"), ("backward_skewed", "pb_skewed")):
        parts = first_positions(w, key) + first_positions(w, "eb")
        nbytes = total * row + B * S * row + 2 * parts * row + 2 * positions * row + 2 * N_BINS * row
        res[name]["partial_sum_rows"] = parts
        res[name]["floor_ms"] = round(nbytes / STREAM_BYTES_PER_S * 1e3, 4)
        res[name]["x_floor"] = round(res[name]["ms"] / res[name]["floor_ms"], 2)
    for name in ("forward", "forward_skewed"):
        res[name]["floor_ms"] = round(fwd_bytes / STREAM_BYTES_PER_S * 1e3, 4)
        res[name]["x_floor"] = round(res[name]["ms"] / res[name]["floor_ms"], 2)
    res["copy"]["gb_per_s"] = round(2 * total * row / res["copy"]["ms"] / 1e6, 1)
    res["forward_over_copy"] = round(res["forward"]["ms"] / res["copy"]["ms"], 3)
    res["backward_over_copy"] = round(res["backward"]["ms"] / res["copy"]["ms"], 3)
    res["pair_over_two_copies"] = round(res["pair"]["ms"] / (2 * res["copy"]["ms"]), 3)
    res["backward_skewed_over_uniform"] = round(res["backward_skewed"]["ms"] / res["backward"]["ms"], 3)
    return res, w, c


def cpu_baseline(w, c):
    import va_ref as R
    one = Calls(w, batch=0)
    one.t["dy"].copy_(c.t["dy"][:one.total])
    one.forward(), one.backward()
    torch.cuda.synchronize()
    sl = slice(0, 1)
    off = np.array([0, one.total], np.int32)
    dy = one.t["dy"].cpu().numpy()
    t = time.perf_counter()
    fw = R.forward(w["x"][sl], w["pb"][sl], w["eb"][sl], w["pt"], w["et"], w["dur"][sl], w["n"][sl], off, one.total)
    bw = R.backward(dy, w["pb"][sl], w["eb"][sl], N_BINS, w["dur"][sl], w["n"][sl], off, one.total)
    s = time.perf_counter() - t
    c.forward(), c.backward()
    for name, got, want in (("frames", c.y[:one.total], fw["y"]), ("dx", c.dx[0], bw["dx"][0]), ("pitch table gradient", one.dpt, bw["d_pitch_table"]),
                            ("energy table gradient", one.det, bw["d_energy_table"]), ("unit_of_frame", c.uof[:one.total], fw["unit_of_frame"])):
        g = got.cpu().numpy()
        if not np.array_equal(g.view(np.int32), np.ascontiguousarray(want).view(np.int32)):
            raise RuntimeError("the GPU and the NumPy restatement disagree on the %s bits of utterance 0" % name)
    return {"what": "NumPy restatement of forward and backward (tests/va_ref.py) on utterance 0 of the full workload on one core, data "
                    "already on the host; scaled by the batch size (not measured at batch size)",
            "frames": one.total, "s_per_utterance": round(s, 4), "s_per_batch_scaled": round(s * B, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-baseline", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_va.py needs a GPU (there is no CPU path)")
    a.runs = max(a.runs, 5)
    rng = np.random.default_rng(1234)
    ragged = [int(t) for t in rng.integers(240, 1001, size=B)]             # bench_f0.py's frame counts
    in_lens = [int(t) for t in np.random.default_rng(4321).integers(40, S + 1, size=B)]
    res = {"bench": "va", "device": torch.cuda.get_device_name(0), "budget_x_copy": BUDGET, "calls_per_timed_interval": REP,
           "stream_bytes_per_s": STREAM_BYTES_PER_S}
    res["full"], w, c = workload([1000] * B, [S] * B, a.runs, a.warmup, 7)
    if a.cpu_baseline:
        res["cpu_baseline"] = cpu_baseline(w, c)
        res["cpu_baseline"]["speedup_vs_full_pair"] = round(res["cpu_baseline"]["s_per_batch_scaled"] * 1e3 / res["full"]["pair"]["ms"])
    del w, c
    torch.cuda.empty_cache()
    res["ragged"] = workload(ragged, in_lens, a.runs, a.warmup, 8)[0]
    res["forward_over_copy"], res["backward_over_copy"] = res["full"]["forward_over_copy"], res["full"]["backward_over_copy"]
    res["within_budget"] = {"forward": res["forward_over_copy"] <= BUDGET, "backward": res["backward_over_copy"] <= BUDGET}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
