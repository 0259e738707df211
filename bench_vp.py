#!/usr/bin/env python3
"""Benchmark of the variance predictor (b2s_hip.predictor: conv, ReLU, LayerNorm, dropout twice, Linear; forward and backward) on
MI355X.

    python bench_vp.py [--runs 20] [--warmup 3] [--cpu-baseline]

Two workloads of 64 utterances with S = 128 positions, D = 768 input columns (the encoder's width), F = 256 filters and p = 0.5:
`full` = 128 positions each, `ragged` = bench_va.py's seeded input lengths of 40..128.

Timed are the library's whole calls on device-resident inputs with outputs, tape and workspace allocated beforehand: `forward`
(b2s_vp_forward with a tape), `backward` (b2s_vp_backward with dx and all ten parameter gradients) and `pair`, one after the other.
The yardstick is measured in the same process: `torch_*` = VariancePredictor.reference_forward, the plain torch composition of the
same submodules in fp32 with torch's own dropout, and its autograd backward (torch.autograd.grad on the retained graph) -- what a user
would otherwise run.  The budget is 1.0x that for the pair.  Every timed interval holds REP calls back to back and is divided by REP.

Derived, not measured: `floor_ms` = the call's FLOPs, 2 x rows x (3 D + 3 F) x F forward and twice that plus the dx term
2 x rows x 3 F x D backward, over the 155 TFLOP/s reported for gfx950's fp32 MFMA.  --cpu-baseline times the NumPy restatement
(tests/vp_ref.py) of forward and backward on utterance 0 of the full workload on one core, checks its bits against the GPU's and
scales it to the batch (labelled as such).  One JSON line.
"""
import argparse
import json
import time

import numpy as np
import torch

from benchtime import stat, time_calls

B, S, D, F, P_DROP, SEED, EPS = 64, 128, 768, 256, 0.5, 20, 1e-5
BUDGET = 1.0
FP32_MFMA_FLOPS = 155e12
REP = 4


class Calls(object):
    """The two C calls on preallocated device tensors, and the torch composition on the same parameters."""

    def __init__(self, in_lens, seed, batch=None):
        from b2s_hip import predictor
        self.p, self.lib = predictor, predictor.load()
        torch.manual_seed(seed)
        self.module = predictor.VariancePredictor(D, F, dropout=P_DROP, eps=EPS).cuda().train()
        with torch.no_grad():
            for norm in (self.module.norm1, self.module.norm2):
                norm.weight.add_(0.2 * torch.randn(F, device="cuda"))
                norm.bias.add_(0.2 * torch.randn(F, device="cuda"))
        gen = torch.Generator(device="cuda").manual_seed(seed)
        x = torch.randn(B, S, D, device="cuda", generator=gen)
        d_pred = torch.randn(B, S, device="cuda", generator=gen)
        n = torch.tensor(in_lens, dtype=torch.int32, device="cuda")
        sl = slice(None) if batch is None else slice(batch, batch + 1)
        self.x, self.d_pred, self.n = x[sl].contiguous(), d_pred[sl].contiguous(), n[sl].contiguous()
        self.nb = int(self.n.numel())
        self.params = [t.detach() for t in self.module.parameters_in_order()]
        self.pred = torch.zeros(self.nb, S, device="cuda")
        self.status = torch.empty(self.nb, dtype=torch.int32, device="cuda")
        self.dx = torch.empty(self.nb, S, D, device="cuda")
        self.grads = [torch.empty_like(t) for t in self.params]
        self.ws_bytes = self.lib.b2s_vp_ws_bytes(self.nb, S, D, F)
        self.tape_bytes = self.lib.b2s_vp_tape_bytes(self.nb, S, F)
        self.ws, self.tape = predictor.workspace(self.ws_bytes, "cuda"), predictor.workspace(self.tape_bytes, "cuda")

    def forward(self):
        self.p.check(self.lib.b2s_vp_forward(self.x.data_ptr(), self.n.data_ptr(), *[t.data_ptr() for t in self.params], EPS, P_DROP, SEED,
                                             self.nb, S, D, F, self.pred.data_ptr(), self.status.data_ptr(), self.tape.data_ptr(),
                                             self.ws.data_ptr(), self.ws_bytes, None))

    def backward(self):
        self.p.check(self.lib.b2s_vp_backward(self.x.data_ptr(), self.n.data_ptr(), *[t.data_ptr() for t in self.params],
                                              self.tape.data_ptr(), self.d_pred.data_ptr(), P_DROP, SEED, self.nb, S, D, F,
                                              self.dx.data_ptr(), *[g.data_ptr() for g in self.grads], self.ws.data_ptr(), self.ws_bytes,
                                              None))

    def outputs(self):
        return [self.pred, self.dx] + self.grads

    def torch_forward(self):
        self.xt = self.x.detach().requires_grad_(True)
        self.torch_pred = self.module.reference_forward(self.xt, self.n)
        return self.torch_pred

    def torch_backward(self):
        return torch.autograd.grad(self.torch_pred, [self.xt] + self.module.parameters_in_order(), self.d_pred, retain_graph=True)


def per_call(fn, runs, warmup):
    def rep():
        for _ in range(REP):
            fn()
    med, lo, hi = time_calls(rep, runs, warmup)
    return stat((med / REP, lo / REP, hi / REP))


def workload(in_lens, runs, warmup, seed):
    c = Calls(in_lens, seed)
    c.forward(), c.backward()
    if c.status.cpu().numpy().any():
        raise RuntimeError("a benchmark utterance is not OK")
    first = [t.clone() for t in c.outputs()]
    c.forward(), c.backward()
    if not all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, c.outputs())):
        raise RuntimeError("the calls do not repeat their bits")
    rows = int(sum(in_lens))
    fwd_flops = 2 * rows * (3 * D + 3 * F) * F
    bwd_flops = 2 * fwd_flops + 2 * rows * 3 * F * D
    res = {"B": B, "S": S, "D": D, "F": F, "p": P_DROP, "rows": rows, "workspace_bytes": c.ws_bytes, "tape_bytes": c.tape_bytes,
           "forward": per_call(c.forward, runs, warmup), "backward": per_call(c.backward, runs, warmup),
           "pair": per_call(lambda: (c.forward(), c.backward()), runs, warmup),
           "torch_forward": per_call(c.torch_forward, runs, warmup)}
    c.torch_forward()
    res["torch_backward"] = per_call(c.torch_backward, runs, warmup)
    res["torch_pair"] = per_call(lambda: (c.torch_forward(), c.torch_backward()), runs, warmup)
    # the composition computes the same function: a loose check that the two were given the same work (dropout off for it)
    c.module.eval()
    with torch.no_grad():
        ref = c.module.reference_forward(c.x, c.n)
        got = c.p.predict(c.x, c.n, c.params, p=0.0)[0]
    c.module.train()
    res["max_abs_diff_to_torch_eval"] = float((ref - got).abs().max())
    for name, flops in (("forward", fwd_flops), ("backward", bwd_flops), ("pair", fwd_flops + bwd_flops)):
        res[name]["flops"] = flops
        res[name]["floor_ms"] = round(flops / FP32_MFMA_FLOPS * 1e3, 4)
        res[name]["x_floor"] = round(res[name]["ms"] / res[name]["floor_ms"], 2)
        res[name]["tflops"] = round(flops / res[name]["ms"] / 1e9, 2)
        res[name + "_over_torch"] = round(res[name]["ms"] / res["torch_" + name]["ms"], 3)
        res["torch_" + name]["tflops"] = round(flops / res["torch_" + name]["ms"] / 1e9, 2)
    res["floors_are_derived"] = True
    return res, c


def cpu_baseline(in_lens, seed, c):
    import vp_ref as R
    one = Calls(in_lens, seed, batch=0)
    one.forward(), one.backward()
    torch.cuda.synchronize()
    P = {k: t.cpu().numpy().reshape(-1) if k == "wl" else t.cpu().numpy() for k, t in zip(c.p.PARAM_NAMES, one.params)}
    x, n, d_pred = one.x.cpu().numpy(), one.n.cpu().numpy(), one.d_pred.cpu().numpy()
    t = time.perf_counter()
    fw = R.forward(x, n, P, EPS, p=P_DROP, seed=SEED)
    bw = R.backward(x, n, P, fw, d_pred)
    s = time.perf_counter() - t
    for name, got, want in (("pred", one.pred, fw["pred"]), ("dx", one.dx, bw["dx"]), ("dW1", one.grads[0], bw["dW1"]),
                            ("dW2", one.grads[4], bw["dW2"]), ("pred in the batch", c.pred[0:1], fw["pred"]),
                            ("dx in the batch", c.dx[0:1], bw["dx"])):
        g = got.cpu().numpy()
        if not np.array_equal(g.view(np.int32), np.ascontiguousarray(want, np.float32).view(np.int32)):
            raise RuntimeError("the GPU and the NumPy restatement disagree on the %s bits of utterance 0" % name)
    return {"what": "NumPy restatement of forward and backward (tests/vp_ref.py) on utterance 0 of the full workload on one core, data "
                    "already on the host; scaled by the batch size (not measured at batch size)",
            "positions": int(n[0]), "s_per_utterance": round(s, 3), "s_per_batch_scaled": round(s * B, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-baseline", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vp.py needs a GPU (there is no CPU path)")
    a.runs = max(a.runs, 5)
    in_lens = [int(t) for t in np.random.default_rng(4321).integers(40, S + 1, size=B)]        # bench_va.py's ragged input lengths
    res = {"bench": "vp", "device": torch.cuda.get_device_name(0), "budget_pair_x_torch": BUDGET, "calls_per_timed_interval": REP,
           "fp32_mfma_flops_per_s": FP32_MFMA_FLOPS}
    res["full"], c = workload([S] * B, a.runs, a.warmup, 7)
    if a.cpu_baseline:
        res["cpu_baseline"] = cpu_baseline([S] * B, 7, c)
        res["cpu_baseline"]["speedup_vs_full_pair"] = round(res["cpu_baseline"]["s_per_batch_scaled"] * 1e3 / res["full"]["pair"]["ms"])
    del c
    torch.cuda.empty_cache()
    res["ragged"] = workload(in_lens, a.runs, a.warmup, 8)[0]
    res["pair_over_torch"] = res["full"]["pair_over_torch"]
    res["within_budget"] = {"pair": res["pair_over_torch"] <= BUDGET}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
