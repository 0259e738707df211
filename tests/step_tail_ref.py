"""float64 restatement of the tail of a training step (TEST INFRASTRUCTURE ONLY; checker of tests/test_gpu_step_tail.py): the loss
(tacotron.py:136-158 as restated by oracle.b2s_oracle.compute_loss), its hand-written gradient, the L2 term over the member set of
oracle.b2s_oracle.l2_member, the fused Adam update in the order of operations of the engine's adam_elem, and the two GEMM images of a postnet
conv weight.  No GPU, no engine imports; plain numpy.  tests/test_step_tail_ref_host.py checks this checker on the CPU.

`dtype=` runs the same statements in float64 (the reference) or in float32 (the honest-fp32 control: every operation rounded to fp32, no fused
multiply-add).  `wrong=` selects ONE deliberately wrong reference (WRONG) for the test of the test.

Bars.  u = 2^-24 is one fp32 rounding (half an ulp, relative).  The DERIVED bars count the roundings of the kernel text (csrc/rowops.hip):

  d_bef, d_aft   k wb (bef - y) with k = 2 / C, wb = w / sum(lens): two divisions, the difference and two products = 5 roundings; each division is
                 allowed 2.5 (a 1-ulp division instead of a correctly rounded one): |err| <= 8 u |ref|.  Rows t >= len are exactly 0.
  l2 backward    g += (reg_weight gscale) p: the scale, the product and the sum = 3 roundings of at most |g| + |a p| each.
  Adam, with A = |g gs| + |l2 p| (>= |g'|; equal to it unless the two terms of g' cancel -- their roundings do not cancel with them):
    g'           two products and a sum: |err| <= 2 u A
    m'           b1 m + (1 - b1) g': two products, a sum, and g': |err| <= 4 u Sm,  Sm = |b1 m| + (1 - b1) A        ((1 - b1) is exact in fp32)
    v'           b2 v + ((1 - b2) g') g': three products, a sum, and g' twice: |err| <= 7 u Sv,  Sv = b2 v + (1 - b2) A^2
    p'           p - (step m') / (sqrt(v') / sbc2 + eps), step = lr / bc1: bc1 and sbc2 arrive rounded (2), the division lr / bc1, the square root, the
                 division by sbc2, the sum with eps, the product and the last division = 8 roundings of |dp|, the error of m' (4 u Sm instead of
                 4 u |m'|: m' may cancel, its error does not), half the relative error of v' (3.5 u Sv / v'), and the final difference (half an ulp of p'):
                 |err| <= 0.5 ulp(p') + u |dp| (8 + 4 Sm / |m'| + 3.5 Sv / v')            -- 0.5 ulp(p') + 15.5 u |dp| where nothing cancels

The MEASURED bars (summation order, atomics, the fast exponential) are 4 x the worst error against float64 over all cases of the GPU test
(profiles/r14_step_tail_parity.json), and never looser than the project's scalar bar 1e-5 + 1e-4 |ref|."""
import zlib

import numpy as np

U = 2.0 ** -24
POS_WEIGHT = 5.0
WRONG_LOSS = ("stop_frame_at_len",         # stop target at frame len instead of len - 1
              "pos_weight_on_negative",    # pos_weight multiplies the negative term
              "divide_by_BT",              # division by B T instead of sum(lens)
              "no_channel_mean",           # squared errors summed, not averaged, over the channels
              "padded_rows_not_zeroed")    # gradient also on rows t >= len
WRONG_ADAM = ("eps_inside_sqrt",           # sqrt(v / bc2 + eps)
              "bc2_without_sqrt",          # sqrt(v) / bc2
              "v_with_g",                  # v' = b2 v + (1 - b2) g'
              "l2_on_layer_norm",          # a LayerNorm weight treated as an L2 member
              "grad_scale_after_l2")       # g' = (g + l2 p) gs
WRONG_CONV = ("no_tap_flip",)              # backward image with tap j instead of 4 - j
WRONG = WRONG_LOSS + WRONG_ADAM + WRONG_CONV

# ----------------------------------------------------------------------------------------------------------------- bars
BAR_DMEL = 8 * U                           # d_bef / d_aft, relative to |ref| element by element
BAR_L2_BWD = 3 * U                         # b2s_l2_backward, relative to |g| + |reg_weight gscale p|
BAR_M, BAR_V = 4 * U, 7 * U                # relative to Sm / Sv
BAR_P_ULP, BAR_P_STEPS = 0.5, 8.0          # see above
SLACK = 1.0 + 2.0 ** -20                   # second-order terms of the first-order bounds above
# measured on one MI355X (profiles/r14_step_tail_parity.json): 4 x the worst value over every case of tests/test_gpu_step_tail.py and over the runs made
CAP_ABS, CAP_REL = 1e-5, 1e-4              # the project's scalar bar (tests/test_gpu_model.py): the measured bars never exceed it
BAR_SCALAR = 8.1e-7                        # out[0..3], out[5]: |err| / |ref|                                  (measured 1.49e-7 to 2.01e-7 from run to run)
BAR_AFT_LOSSES = 4.9e-7                    # aft_losses: |err| / |ref|                                          (measured 1.21e-7)
BAR_L2 = 7.6e-7                            # out[4] on both routes: |err| / |ref|          (measured 1.0e-7 to 1.89e-7 recomputed -- atomics --, 4.4e-8 from the chunk sums)
BAR_DSTOP = 3.4e-7                         # d_stop: |err| / (pos_weight w / sum(lens)), the largest magnitude an element can have   (measured 8.4e-8)
ADAM_BITWISE = True                        # every Adam case agreed bit for bit with the float32 restatement on the GPU -> asserted


def bf16_rne(x):
    """float -> nearest bfloat16 (ties to even), returned as float32."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def l2_member(name):
    """tacotron.py:144-146: which parameters enter the L2 term."""
    return ("weight" in name and "layer_norm" not in name and "batchnorm" not in name
            and "encoder.speaker_embed" not in name and "encoder.embed" not in name)


def member_fn(wrong=None):
    if wrong == "l2_on_layer_norm":
        return lambda n: l2_member(n) or ("layer_norm" in n and "weight" in n)
    return l2_member


# ----------------------------------------------------------------------------------------------------------------- loss
def _softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def _valid(lens, T):
    return np.arange(T)[None, :] < np.asarray(lens)[:, None]


def loss(bef, aft, stop, tgt, lens, l2, dtype=np.float64, wrong=None):
    """-> (out[7] = loss, bef_loss, aft_loss, mse_loss, l2, stop_loss, sum(lens); aft_losses[B])."""
    assert wrong is None or wrong in WRONG_LOSS
    f = dtype
    bef, aft, stop, tgt = (np.asarray(a, dtype=f) for a in (bef, aft, stop, tgt))
    lens = np.asarray(lens, dtype=np.int64)
    B, T, C = tgt.shape
    valid = _valid(lens, T)
    sl = f(B * T) if wrong == "divide_by_BT" else f(lens.sum())
    chan = (lambda e: e.sum(-1)) if wrong == "no_channel_mean" else (lambda e: e.sum(-1) / f(C))
    eb, ea = chan((bef - tgt) ** 2), chan((aft - tgt) ** 2)                  # [B, T]
    lb = np.where(valid, eb, f(0)).sum(dtype=f) / sl
    per = np.where(valid, ea, f(0)).sum(-1, dtype=f)
    la = per.sum(dtype=f) / sl
    stop_at = lens if wrong == "stop_frame_at_len" else lens - 1
    is_stop = np.arange(T)[None, :] == stop_at[:, None]
    pos, neg = _softplus(-stop), _softplus(stop)
    pw = f(POS_WEIGHT)
    ce_e = np.where(is_stop, pos, pw * neg) if wrong == "pos_weight_on_negative" else np.where(is_stop, pw * pos, neg)
    ce = np.where(valid, ce_e, f(0)).sum(dtype=f) / sl
    l2 = f(l2)
    out = np.array([lb + la + l2 + ce, lb, la, (lb + la) * f(0.5), l2, ce, f(lens.sum())], dtype=f)
    return out, (per / lens.astype(f)).astype(f)


def loss_grads(bef, aft, stop, tgt, lens, w3=None, dtype=np.float64, wrong=None):
    """Hand-written gradients of w3[0] bef_loss + w3[1] aft_loss + w3[2] stop_loss -> (d_bef, d_aft, d_stop); exactly zero on rows t >= len."""
    assert wrong is None or wrong in WRONG_LOSS
    f = dtype
    bef, aft, stop, tgt = (np.asarray(a, dtype=f) for a in (bef, aft, stop, tgt))
    lens = np.asarray(lens, dtype=np.int64)
    B, T, C = tgt.shape
    w = np.ones(3, dtype=f) if w3 is None else np.asarray(w3, dtype=f)
    sl = f(B * T) if wrong == "divide_by_BT" else f(lens.sum())
    wb, wa, ws = w[0] / sl, w[1] / sl, w[2] / sl
    valid = _valid(lens, T)
    k = f(2) if wrong == "no_channel_mean" else f(2) / f(C)
    kk = np.where(valid, k, f(0)) if wrong != "padded_rows_not_zeroed" else np.full(valid.shape, k, dtype=f)
    d_bef = (kk * wb)[:, :, None] * (bef - tgt)
    d_aft = (kk * wa)[:, :, None] * (aft - tgt)
    sg = f(1) / (f(1) + np.exp(-stop))
    stop_at = lens if wrong == "stop_frame_at_len" else lens - 1
    is_stop = np.arange(T)[None, :] == stop_at[:, None]
    pw = f(POS_WEIGHT)
    g = np.where(is_stop, -(f(1) - sg), pw * sg) if wrong == "pos_weight_on_negative" else np.where(is_stop, -pw * (f(1) - sg), sg)
    d_stop = g * ws
    if wrong != "padded_rows_not_zeroed":
        d_stop = np.where(valid, d_stop, f(0))
    return d_bef.astype(f), d_aft.astype(f), d_stop.astype(f)


# ----------------------------------------------------------------------------------------------------------------- L2
def l2_value(params, reg_weight, member=l2_member):
    """reg_weight sum over the members of sum(p^2) / 2, float64.  params: {name: array}, parameters only."""
    return float(reg_weight) * sum(float((np.asarray(p, dtype=np.float64) ** 2).sum()) / 2.0 for n, p in params.items() if member(n))


def l2_grad(params, reg_weight, gscale=1.0, member=l2_member):
    """{name: reg_weight gscale p} for the members, float64 (what b2s_l2_backward adds to their gradients)."""
    return {n: float(reg_weight) * float(gscale) * np.asarray(p, dtype=np.float64) for n, p in params.items() if member(n)}


# ----------------------------------------------------------------------------------------------------------------- Adam
def adam_hyper(lr, step, b1, b2, dtype=np.float64):
    """(step size lr / bc1, sbc2 = sqrt(1 - b2^t)).  float32: the bias corrections are computed in double and rounded once, then lr / bc1 in fp32
    (what the kernel is handed and does)."""
    f = dtype
    bc1, sbc2 = 1.0 - float(b1) ** int(step), np.sqrt(1.0 - float(b2) ** int(step))
    return f(lr) / f(bc1), f(sbc2)


def adam(p, g, m, v, lr, step, b1, b2, eps, l2, grad_scale, member, dtype=np.float64, wrong=None):
    """One update of adam_elem on arrays: g' = g gs + l2 p for members (member: bool, scalar or array), m' = b1 m + (1 - b1) g',
    v' = b2 v + ((1 - b2) g') g', p' = p - (step m') / (sqrt(v') / sbc2 + eps).  -> (p', m', v')."""
    assert wrong is None or wrong in WRONG_ADAM
    f = dtype
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    b1, b2, eps, gs = f(b1), f(b2), f(eps), f(grad_scale)
    l2p = np.where(member, f(l2), f(0)).astype(f)
    stp, sbc2 = adam_hyper(lr, step, b1, b2, f)
    gp = (g + l2p * p) * gs if wrong == "grad_scale_after_l2" else g * gs + l2p * p
    m1 = b1 * m + (f(1) - b1) * gp
    v1 = b2 * v + ((f(1) - b2) * gp if wrong == "v_with_g" else ((f(1) - b2) * gp) * gp)
    if wrong == "eps_inside_sqrt":
        den = np.sqrt(v1 / (sbc2 * sbc2) + eps)
    elif wrong == "bc2_without_sqrt":
        den = np.sqrt(v1) / (sbc2 * sbc2) + eps
    else:
        den = np.sqrt(v1) / sbc2 + eps
    p1 = p - (stp * m1) / den
    return p1.astype(f), m1.astype(f), v1.astype(f)


def adam_bars(p, g, m, v, lr, step, b1, b2, eps, l2, grad_scale, member):
    """Element-wise bars of p', m', v' against adam(dtype=float64) (module docstring).  -> (bar_p, bar_m, bar_v), float64 arrays."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    l2p = np.where(member, float(l2), 0.0)
    A = np.abs(g * grad_scale) + np.abs(l2p * p)
    p1, m1, v1 = adam(p, g, m, v, lr, step, b1, b2, eps, l2, grad_scale, member)
    Sm = np.abs(b1 * m) + (1.0 - b1) * A
    Sv = b2 * v + (1.0 - b2) * A * A
    stp, sbc2 = adam_hyper(lr, step, b1, b2)
    k = np.abs(stp) / (np.sqrt(v1) / sbc2 + eps)                        # |dp| = k |m'|
    with np.errstate(divide="ignore", invalid="ignore"):
        rv = np.where(v1 > 0, Sv / v1, 0.0)
    ulp = np.spacing(np.maximum(np.abs(p1), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
    bar_p = BAR_P_ULP * ulp + U * k * (BAR_P_STEPS * np.abs(m1) + BAR_M / U * Sm + 0.5 * BAR_V / U * rv * np.abs(m1))
    return bar_p * SLACK, BAR_M * Sm * SLACK, BAR_V * Sv * SLACK


# ----------------------------------------------------------------------------------------------------------------- conv images
def conv_images(w, wrong=None):
    """w [Cout, Cin, 5] -> (fwd [Cout, 5 Cin] with fwd[co][j Cin + ci] = w[co][ci][j], bwd [Cin, 5 Cout] with bwd[ci][(4 - j) Cout + co] = w[co][ci][j])."""
    assert wrong is None or wrong in WRONG_CONV
    w = np.asarray(w)
    Cout, Cin, K = w.shape
    assert K == 5
    fwd = w.transpose(0, 2, 1).reshape(Cout, 5 * Cin)
    wb = w if wrong == "no_tap_flip" else w[:, :, ::-1]
    bwd = wb.transpose(1, 2, 0).reshape(Cin, 5 * Cout)
    return np.ascontiguousarray(fwd), np.ascontiguousarray(bwd)


# ----------------------------------------------------------------------------------------------------------------- cases shared by the host and the GPU tests
# id -> (num_mels, B, T, lens): the smallest shapes that reach each branch of k_loss_partial_v (grid x = min(ceil(T C / 4 / 1024), 16) workgroups of 256
# threads per utterance, stride = 256 x; each thread takes float4 i0, i0 + stride, i0 + 2 stride, i0 + 3 stride per trip, indices clamped to n4 - 1)
LOSS_CASES = {
    "one-frame": (80, 1, 1, (1,)),                            # the only frame is the stop frame
    "golden": (80, 3, 23, (23, 15, 9)),                       # the shape of test_forward_loss_grads_fp32
    "two-wg": (80, 2, 52, (52, 51)),                          # T C / 4 = 1040: the grid goes from 1 to 2 workgroups
    "partial-unroll": (80, 4, 205, (205, 204, 1, 103)),       # 5 workgroups, n4 = 4100 < 4 stride = 5120: the unrolled loads run past n4
    "second-trip": (80, 2, 820, (820, 819)),                  # 16 workgroups; n4 = 16400 / 16380 straddle 4 stride = 16384: second trip of 16 float4, clamp live
    "many": (80, 33, 3, tuple(1 + (5 * i) % 3 for i in range(33))),      # 33 utterances of 1..3 frames: 3 + B accumulators
    "mels8": (8, 5, 7, (7, 1, 4, 2, 6)),                      # num_mels = 8: n4 of 2..14
}
W3 = (None, (0.5, 2.0, 3.0))
STOP_SPECIALS = (0.0, 30.0, -30.0, 88.0, -88.0)
ADAM_STEPS, ADAM_SCALES = (1, 7, 100000), (1.0, 0.5)
BETA1, BETA2 = float(np.float32(0.9)), float(np.float32(0.999))


def loss_inputs(case):
    """(bef, aft, stop, tgt) fp32 and lens: O(1) values with a non-zero mean, about 3 % of the predictions equal to the target bit for bit, the stop
    logits 0, +-30 and +-88 at stop frames and at other frames, and large finite values on every padded row (the masks have to remove them)."""
    C, B, T, lens = LOSS_CASES[case]
    g = np.random.default_rng(zlib.crc32(case.encode()))
    lens = np.asarray(lens, dtype=np.int64)
    tgt = (0.5 + g.standard_normal((B, T, C))).astype(np.float32)
    bef = (tgt + 0.1 + 0.3 * g.standard_normal((B, T, C))).astype(np.float32)
    aft = (tgt - 0.05 + 0.2 * g.standard_normal((B, T, C))).astype(np.float32)
    bef = np.where(g.random((B, T, C)) < 0.03, tgt, bef)
    aft = np.where(g.random((B, T, C)) < 0.03, tgt, aft)
    stop = (2.0 * g.standard_normal((B, T))).astype(np.float32)
    k = 0
    for b in range(B):
        stop[b, lens[b] - 1] = STOP_SPECIALS[k % 5] if (b % 2 == 0 or B < 3) else stop[b, lens[b] - 1]
        k += 1
        for t in range(0, int(lens[b]) - 1, max(1, int(lens[b]) // 6)):
            stop[b, t] = STOP_SPECIALS[k % 5]
            k += 1
    pad = ~_valid(lens, T)
    bef[pad] = 100.0 * g.standard_normal((int(pad.sum()), C)).astype(np.float32)
    aft[pad] = -100.0 + 0 * aft[pad]
    tgt[pad] = 50.0 * g.standard_normal((int(pad.sum()), C)).astype(np.float32)
    stop[pad] = 88.0
    return bef, aft, stop, tgt, lens


def adam_inputs(name, n, seed=0):
    """(p, g, m, v) fp32 [n] of one tensor, seeded by its name.  |p| spreads over 4 decades and |g| over 6; |m| lies within a decade of |g| and v within
    two decades of g^2 (so that no element moves by more than about 0.1 and the L2 value after the step is not the square of a few runaway elements),
    m has the sign opposite to g on about a third of the elements, g = 0 and v = 0 on about 5 % each and both on a further 1 %."""
    r = np.random.default_rng([zlib.crc32(name.encode()), seed])
    sign = lambda: np.where(r.random(n) < 0.5, -1.0, 1.0)
    p = sign() * 10.0 ** r.uniform(-4, 0, n)
    g = sign() * 10.0 ** r.uniform(-6, 0, n)
    m = np.where(r.random(n) < 0.35, -g, g) * 10.0 ** r.uniform(-1, 1, n)
    v = g * g * 10.0 ** r.uniform(-2, 2, n)
    both = r.random(n) < 0.01
    zg, zv = (r.random(n) < 0.05) | both, (r.random(n) < 0.05) | both
    m = np.where(zg & zv, 1e-7 * np.sign(m) * r.random(n), m)          # (the step of such an element is step m / eps)
    g = np.where(zg, 0.0, g)
    v = np.where(zv, 0.0, v)
    return tuple(a.astype(np.float32) for a in (p, g, m, v))


def rel_err(got, ref):
    """max |got - ref| / |ref| over the elements (0 / 0 = 0)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    d = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d == 0, 0.0, d / np.abs(ref))
    return float(np.max(q)) if q.size else 0.0


def loss_excess(got, ref, w3=None):
    """{kind: (error / its bar, error in the unit of the bar)} of a loss result.  got / ref: dict with any of out [7], aft_losses [B], d_bef, d_aft,
    d_stop (+ lens for d_stop).  out[4] (the L2 value) is not judged here: the caller compares it with l2_value of the current masters."""
    res = {}
    if "out" in ref:
        idx = [0, 1, 2, 3, 5]
        e = rel_err(np.asarray(got["out"])[idx], np.asarray(ref["out"])[idx])
        res["scalar"] = (e / BAR_SCALAR, e)
        res["sum_lens"] = (0.0 if float(got["out"][6]) == float(ref["out"][6]) else float("inf"), abs(float(got["out"][6]) - float(ref["out"][6])))
    if "aft_losses" in ref:
        e = rel_err(got["aft_losses"], ref["aft_losses"])
        res["aft_losses"] = (e / BAR_AFT_LOSSES, e)
    for k in ("d_bef", "d_aft"):
        if k in ref:
            e = rel_err(got[k], ref[k])
            res[k] = (e / BAR_DMEL, e)
    if "d_stop" in ref:
        ws = (1.0 if w3 is None else float(w3[2])) / float(np.sum(ref["lens"]))
        e = float(np.max(np.abs(np.asarray(got["d_stop"], dtype=np.float64) - ref["d_stop"]))) / (POS_WEIGHT * ws)
        res["d_stop"] = (e / BAR_DSTOP, e)
    return res
