"""float64 restatement of the postnet segment with hooks (TEST INFRASTRUCTURE ONLY; checker of tests/test_gpu_postnet.py).

Follows oracle/b2s_oracle.py: postnet_forward (tacotron.py:81-90): n x {length mask, Conv1d k5 p2 without bias, BatchNorm1d over ALL B T
positions, tanh except on the last layer, dropout}, channels-last [B, T, C] like the engine.  Two things the oracle cannot do:

  masks=   the engine's dropout keep-masks (oracle/rng.py: DeviceMasks; site "postnet.conv", flat index over [B, T, C]) -- used by the forward and,
           again, by the hand-written backward (the engine regenerates them there).
  round=   a function applied exactly where the bf16 engine stores bf16: the layer inputs u[i] (the cast input and every post-tanh / dropout
           activation), the conv weight images, and in the backward dy[i] (BatchNorm-backward output) and du[i], i > 0 (backward-data output).
           The conv outputs y, the statistics, dgamma, dbeta, dW and the layer-0 d_inputs stay unrounded (fp32 in the engine).

The backward is written out by hand so that these roundings can be inserted; with round=None and masks=None the forward equals
O.postnet_forward and the backward torch autograd of it (tests/test_postnet_ref_host.py).

`wrong=` selects ONE deliberately wrong reference (WRONG below) for the test of the test: the bars must tell each of them from the right one."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
MOMENTUM = 0.1
WRONG = ("stats_valid_rows",        # statistics over the valid rows only instead of all B T rows
         "biased_running_var",      # running variance without the M / (M - 1) factor
         "reversed_taps",           # filter taps applied in reversed order
         "no_length_mask",          # no length mask before the conv of layers >= 1
         "tanh_last",               # tanh applied on the last layer too
         "no_dgamma_dbeta")         # dy = gamma rstd dz: the two mean terms of the BatchNorm backward dropped


def _f64(a):
    return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).detach().to(torch.float64)


def _rounder(round):
    if round is None:
        return lambda t: t
    return lambda t: round(t).to(torch.float64)


def _keep_scale(masks, layer, shape, p):
    """keep * 1 / (1 - p) the way the engine scales (fp32 quotient), or None with dropout off."""
    if masks is None or p <= 0.0:
        return None
    keep = torch.from_numpy(masks.keep("postnet.conv", layer, tuple(shape), p))
    return keep.to(torch.float64) * float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def _conv(u, w):
    """[B, T, Cin] x [Cout, Cin, 5] -> [B, T, Cout], zero padding 2 per utterance."""
    return F.conv1d(u.transpose(1, 2), w, None, 1, 2).transpose(1, 2)


def forward(P, cfg, inputs, lengths, train=True, masks=None, round=None, add_inputs=False, wrong=None):
    """-> dict: y (list of conv outputs [B, T, Cout]), out [B, T, num_mels] (+ inputs if add_inputs), bn_state (the updated
    running_mean / running_var / num_batches_tracked; empty in eval mode), ctx (what backward() needs)."""
    assert wrong is None or wrong in WRONG
    rnd = _rounder(round)
    n = cfg.n_postnet_layer
    p = cfg.decoder_dropout_rate if train else 0.0
    x = _f64(inputs)
    B, T, _ = x.shape
    M = B * T
    valid = (torch.arange(T)[None, :] < torch.as_tensor(lengths).long()[:, None])          # [B, T]
    vm = valid.to(torch.float64)[:, :, None]
    ctx = dict(n=n, M=M, vm=vm, wrong=wrong, rnd=rnd, u=[], w=[], xhat=[], rstd=[], gamma=[], a=[], ks=[])
    ys, bn_state = [], {}
    u = rnd(x)
    for i in range(n):
        w = rnd(_f64(P["postnet.conv_layers.%d.weight" % i]))
        if wrong == "reversed_taps":
            w = w.flip(2)
        um = u if (wrong == "no_length_mask" and i > 0) else u * vm
        y = _conv(um, w)
        ys.append(y)
        q = "postnet.batchnorm_layers.%d." % i
        gamma, beta = _f64(P[q + "weight"]), _f64(P[q + "bias"])
        if train:
            if wrong == "stats_valid_rows":
                rows = y[valid]
                mean, var, cnt = rows.mean(0), rows.var(0, unbiased=False), rows.shape[0]
            else:
                mean, var, cnt = y.mean(dim=(0, 1)), y.var(dim=(0, 1), unbiased=False), M
            unb = 1.0 if wrong == "biased_running_var" else cnt / (cnt - 1.0)
            bn_state[q + "running_mean"] = (1 - MOMENTUM) * _f64(P[q + "running_mean"]) + MOMENTUM * mean
            bn_state[q + "running_var"] = (1 - MOMENTUM) * _f64(P[q + "running_var"]) + MOMENTUM * var * unb
            bn_state[q + "num_batches_tracked"] = torch.as_tensor(P[q + "num_batches_tracked"]).long() + 1
        else:
            mean, var = _f64(P[q + "running_mean"]), _f64(P[q + "running_var"])
        rstd = 1.0 / torch.sqrt(var + EPS)
        xhat = (y - mean) * rstd
        z = xhat * gamma + beta
        use_tanh = i != n - 1 or wrong == "tanh_last"
        a = torch.tanh(z) if use_tanh else z
        ks = _keep_scale(masks, i, a.shape, p)
        o = a if ks is None else a * ks
        for k, v in (("u", um), ("w", w), ("xhat", xhat), ("rstd", rstd), ("gamma", gamma), ("a", a if use_tanh else None), ("ks", ks)):
            ctx[k].append(v)
        if i != n - 1:
            u = rnd(o)                                   # stored in the compute dtype; the last layer's output is fp32
    out = o + x if add_inputs else o
    return {"y": ys, "out": out, "bn_state": bn_state, "ctx": ctx}


def backward(res, grad_out):
    """Hand-written backward of a train-mode forward().  -> dict: d_inputs [B, T, num_mels] (without the `+ grad_out` of add_inputs),
    dW / dgamma / dbeta (lists per layer)."""
    c = res["ctx"]
    n, M, vm, rnd = c["n"], c["M"], c["vm"], c["rnd"]
    dW, dgamma, dbeta = [None] * n, [None] * n, [None] * n
    d = _f64(grad_out)
    for i in range(n - 1, -1, -1):
        if c["ks"][i] is not None:
            d = d * c["ks"][i]                           # the mask of the forward, regenerated
        if c["a"][i] is not None:
            d = d * (1.0 - c["a"][i] ** 2)
        xhat, g = c["xhat"][i], c["gamma"][i] * c["rstd"][i]
        dbeta[i] = d.sum(dim=(0, 1))
        dgamma[i] = (d * xhat).sum(dim=(0, 1))
        if c["wrong"] == "no_dgamma_dbeta":
            dy = g * d
        else:
            dy = g * (d - dbeta[i] / M - xhat * dgamma[i] / M)
        dy = rnd(dy)
        um, w = c["u"][i], c["w"][i]
        up = F.pad(um, (0, 0, 2, 2))                     # dW[co, ci, j] = sum_{b,t} dy[b, t, co] u[b, t + j - 2, ci]
        T = um.shape[1]
        dW[i] = torch.stack([torch.einsum("bto,bti->oi", dy, up[:, j:j + T]) for j in range(5)], dim=2)
        dx = F.conv_transpose1d(dy.transpose(1, 2), w, None, 1, 2).transpose(1, 2)
        if not (c["wrong"] == "no_length_mask" and i > 0):
            dx = dx * vm
        d = rnd(dx) if i > 0 else dx
    return {"d_inputs": d, "dW": dW, "dgamma": dgamma, "dbeta": dbeta}


def step(P, cfg, x, lengths, grad_out, **kw):
    """forward() + backward() under the names the tests compare: out, x.grad, <parameter>.grad, the updated running statistics."""
    r = forward(P, cfg, x, lengths, train=True, **kw)
    g = backward(r, grad_out)
    res = {"out": r["out"], "x.grad": g["d_inputs"]}
    for i in range(cfg.n_postnet_layer):
        res["conv_layers.%d.weight.grad" % i] = g["dW"][i]
        res["batchnorm_layers.%d.weight.grad" % i] = g["dgamma"][i]
        res["batchnorm_layers.%d.bias.grad" % i] = g["dbeta"][i]
    for k, v in r["bn_state"].items():
        res[k[len("postnet."):]] = v
    return res


def kind_of(name):
    return "out" if name == "out" else "grad" if name.endswith(".grad") else "nbt" if name.endswith("num_batches_tracked") else "stat"


def excess(got, ref, bf16=False):
    """{name: (error / its bar, error)} for every tensor of `ref`.  fp32 bars: max |err| against BAR_ACT, BAR_GRAD * max(1, ||ref||_2), BAR_STAT.
    bf16 bars: max |err| / max |ref| (gpu_util.relerr) against BAR16_*.  num_batches_tracked: exact."""
    out = {}
    for k, r in ref.items():
        g, kind = got[k], kind_of(k)
        if kind == "nbt":
            out[k] = (0.0 if int(g) == int(r) else float("inf"), abs(int(g) - int(r)))
            continue
        g, r = g.detach().double().cpu(), r.double()
        assert g.shape == r.shape, (k, g.shape, r.shape)
        err = float((g - r).abs().max())
        if not np.isfinite(err):
            out[k] = (float("inf"), err)
        elif bf16:
            err = err / (float(r.abs().max()) + 1e-12)
            out[k] = (err / {"out": BAR16_OUT, "grad": BAR16_GRAD, "stat": BAR16_STAT}[kind], err)
        else:
            out[k] = (err / {"out": BAR_ACT, "grad": BAR_GRAD * max(1.0, float(r.norm())), "stat": BAR_STAT}[kind], err)
    return out


# --------------------------------------------------------------------------- cases and bars shared by the host and the GPU tests
# id -> (num_mels, postnet_hidden, n_postnet_layer, B, T, lengths): the smallest shapes that reach each edge of the kernels
CASES = {
    "A": (80, 48, 3, 3, 23, (23, 15, 9)),          # anchor: the golden shape
    "B": (80, 48, 3, 4, 70, (70, 69, 2, 1)),       # 280 rows: 256-row tile kernel + edge block, utterance boundaries inside a tile, segments shorter than the tap reach
    "C": (8, 8, 3, 1, 31, (31,)),                  # smallest channel count (2 owning lanes, 62 clamped); one row short of a 32-row block
    "D": (8, 264, 3, 2, 16, (16, 5)),              # exactly one 32-row block; second channel workgroup owning 2 quads
    "E": (16, 512, 3, 3, 11, (11, 10, 1)),         # 33 rows; two full channel workgroups; length 1
    "F": (80, 512, 3, 2, 129, (129, 65)),          # 258 rows; aligned 512-channel conv gather of the 256-row kernel; length 64 + 1
    "G": (80, 48, 3, 1, 128, (128,)),              # exactly one 128-row tile, no padding at all
    "H": (80, 48, 3, 2, 1, (1, 1)),                # T = 1 (only the centre tap sees data), M = 2: forward and running statistics only
    "I": (80, 48, 1, 3, 23, (23, 15, 9)),          # first layer is also the last: fp32 dout, no tanh, fp32 d_inputs
    "J": (80, 48, 3, 1, 64, (64,)),                # 64 rows: the last row count whose batch variance is taken two-pass (rowops.hip: BN_TWO_PASS_M)
    "K": (80, 48, 3, 5, 13, (13, 12, 1, 13, 7)),   # 65 rows: the first that keeps the one-pass variance of the GEMM epilogue's column sums
}

# fp32 bars: the project's own (tests/test_gpu_model.py, tests/test_gpu_conv_dw_segments.py)
BAR_ACT = 2e-4            # max |err| of activations
BAR_GRAD = 2e-4           # max |err| <= BAR_GRAD * max(1, ||ref||_2) for x.grad and every parameter gradient
BAR_STAT = 1e-5           # running_mean / running_var
# bf16 bars against the ROUNDED restatement (identical operands: accumulation order and one-ulp rounding flips remain), gpu_util.relerr
# (out and statistics tightened from TOL[1] = 1e-2 of tests/test_gpu_ops.py and 1e-3: measured 2.5e-4 and 5.8e-6, more than 20 x below; not to 4 x the
# measurement but to what the rounded restatement itself differs from plain float64 by, 4.9e-3 and 3.4e-4 -- the rounding flips that can differ)
BAR16_OUT = 5e-3
BAR16_GRAD = 3e-2         # the bf16 gradient bar of test_attention_core_fwd_bwd (measured 3.7e-3)
BAR16_STAT = 3.5e-4       # running statistics, relative to the largest reference entry


def case_over(case, dropout=0.0):
    """hparams override string of a case: TINY with one encoder and one decoder layer and the case's postnet."""
    from oracle import TINY
    nm, hid, nl = CASES[case][:3]
    over = TINY
    for old, new in (("n_encoder_layer=2", "n_encoder_layer=1"), ("n_decoder_layer=2", "n_decoder_layer=1"),
                     ("postnet_hidden=48", "postnet_hidden=%d" % hid), ("n_postnet_layer=3", "n_postnet_layer=%d" % nl),
                     (",decoder_dropout_rate=0.0", ",decoder_dropout_rate=%s" % dropout)):
        assert old in over
        over = over.replace(old, new)
    return over + ",num_mels=%d" % nm


def case_inputs(case, seed=0):
    """(x [B, T, num_mels] fp32, lengths int64 [B], grad_out fp32): N(0, 1) on every row, padded rows included (the length mask has to
    remove them)."""
    nm, _, _, B, T, lens = CASES[case]
    g = torch.Generator().manual_seed(1000 + 7 * seed + sum(map(ord, case)))
    x = torch.randn(B, T, nm, generator=g)
    go = torch.randn(B, T, nm, generator=g)
    return x, torch.tensor(lens, dtype=torch.int64), go


def channel_ratio(y):
    """worst channel |mean| / std of a conv output over all B T rows."""
    y = y.reshape(-1, y.shape[-1])
    return float((y.mean(0).abs() / y.std(0, unbiased=False)).max())


# The one-pass batch variance sum(y^2) / M - mean^2: inputs x = c + s N(0, 1) over the 280 rows of case B whose layer-0 conv output has a given worst
# channel |mean| / std.  Two things bound that ratio whatever c is.  A padded row's conv output is 0, so with a fraction f of valid rows it cannot
# exceed sqrt(f / (1 - f)): about 1 at case B's own lengths (142 of 280 rows valid).  And the two rows at either end of an utterance miss taps, so they
# sit off the channel mean by a multiple of c: four utterances of 70 frames stop near 18.  "mel-like" keeps case B's lengths; "offset" leaves one
# padded row; "beyond" is one utterance of 280 frames -- the same 280 rows (256-row tile + edge block), or its band could not be reached.
OFFSET_INPUTS = {            # name -> (B, T, lengths, band, target ratio or None = the mel statistics c = 0.55, s = 0.58)
    "mel-like": (4, 70, (70, 69, 2, 1), (0.3, 4.0), None),
    "offset": (4, 70, (70, 70, 70, 69), (6.0, 10.0), 8.0),
    "beyond": (1, 280, (280,), (28.0, 36.0), 32.0),
}


def offset_input(name, P, cfg):
    """(x, lengths, grad_out, band, (c, s)) of one of OFFSET_INPUTS.  c is chosen on the CPU: the ratio of the fp64 layer-0 conv output grows
    with c, so c is bisected (on a log scale) to the target."""
    B, T, lens, band, target = OFFSET_INPUTS[name]
    nm = CASES["B"][0]
    g = torch.Generator().manual_seed(4242)
    noise = torch.randn(B, T, nm, generator=g).double()
    go = torch.randn(B, T, nm, generator=g)
    lengths = torch.tensor(lens, dtype=torch.int64)
    vm = (torch.arange(T)[None, :] < lengths[:, None]).double()[:, :, None]
    w0 = _f64(P["postnet.conv_layers.0.weight"])
    s = 0.58
    ratio = lambda c: channel_ratio(_conv((c + s * noise) * vm, w0))
    if target is None:
        c = 0.55
    else:
        lo, hi = 1e-2, 1e4
        for _ in range(40):
            c = (lo * hi) ** 0.5
            lo, hi = (c, hi) if ratio(c) < target else (lo, c)
    return (c + s * noise).float(), lengths, go, band, (c, s)
