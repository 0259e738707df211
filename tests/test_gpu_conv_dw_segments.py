"""Conv1d(k = 5, pad = 2) weight gradients on per-utterance K segments (no gathered operand): the grouped bf16 weight-gradient
kernel walks, for every filter tap, the rows of dy and the row-shifted rows of the conv input utterance by utterance.

Expected values: torch's conv1d weight gradient in fp64 on the CPU, on the same bf16-rounded operands, with the conv input zeroed on
the rows at or beyond the utterance length (the reference semantics: `impute` before every conv) and dy kept on ALL rows.  On the
device those input rows hold NaN instead of zeros: the kernel must never read them, a single read poisons the result.

Bar: the one tests/test_gpu_model.py applies to the `postnet.conv_layers.*.weight` gradients, max |error| <= 2e-4 * max(1, |ref|_2).
The only error source at the op level is the fp32 accumulation order (operands are identical), far below that.
The end-to-end case runs the bf16 postnet against the fp32 oracle: there the operands themselves are bf16-rounded activations, and the
bar is the bf16 one of the same file (worst relative gradient-norm error, drift_gate ceiling 0.06).
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import b2s_oracle as O                     # checker only
from oracle import TINY
from gpu_util import DEV, bf16_round, to_dev_compute, drift_gate

SHAPE_A = (4, 70, (70, 69, 2, 1))        # full-length utterance next to its neighbour, first / last rows of the buffers, segments shorter than the tap reach
SHAPE_B = (3, 150, (150, 64, 65))        # exact and off-by-one multiples of the 64-deep K step
CASES = [(SHAPE_A, 32, 32), (SHAPE_A, 80, 64), (SHAPE_A, 64, 80), (SHAPE_A, 512, 512), (SHAPE_B, 32, 32), (SHAPE_B, 64, 80)]
IDS = ["B%dT%d-%dx%d" % (s[0], s[1], ci, co) for s, ci, co in CASES]


@functools.lru_cache(maxsize=None)
def operands(shape, cin, cout, masked=True):
    """(dy, x, fp64 reference [cout][cin][5]) -- computed once per case and shared; callers do not modify them."""
    B, T, lens = shape
    g = torch.Generator().manual_seed(1000 * cin + cout + T)
    dy = bf16_round(torch.randn(B, T, cout, generator=g))
    x = bf16_round(torch.randn(B, T, cin, generator=g))
    xz = x.clone()
    if masked:
        for b, n in enumerate(lens):
            xz[b, n:] = 0.0
    ref = torch.nn.grad.conv1d_weight(xz.double().transpose(1, 2), (cout, cin, 5), dy.double().transpose(1, 2), padding=2)
    return dy, x, ref


def run(shape, cin, cout, init=None, masked=True):
    from b2s_hip import ops
    B, T, lens = shape
    dy, x, ref = operands(shape, cin, cout, masked)
    xd = x.clone()
    if masked:
        for b, n in enumerate(lens):
            xd[b, n:] = float("nan")                   # never read
    A = to_dev_compute(dy.reshape(B * T, cout), 1)
    Bm = to_dev_compute(xd.reshape(B * T, cin), 1)
    out = None if init is None else init.clone().to(DEV)
    ln = torch.tensor(lens, dtype=torch.int32, device=DEV) if masked else None
    got = ops.gemm(1, A, Bm, cout, 5 * cin, B * T, trans_a=True, trans_b=True, out=out, lda=cout, ldb=cin, ldc=5 * cin,
                   accumulate=init is not None, conv_T=T, conv_len=ln, conv_dw_cin=cin)
    torch.cuda.synchronize()
    return got.cpu().double().reshape(cout, cin, 5), ref


def check(got, ref, what):
    err = float((got - ref).abs().max())
    bar = 2e-4 * max(1.0, float(ref.norm()))
    print("%s: max|err| = %.3e, bar = %.3e, |ref|_2 = %.3e" % (what, err, bar, float(ref.norm())))
    assert torch.isfinite(got).all(), what
    assert err <= bar, (what, err, bar)


@pytest.mark.parametrize("shape,cin,cout", CASES, ids=IDS)
def test_conv_dw_segments_match_fp64(shape, cin, cout):
    got, ref = run(shape, cin, cout)
    check(got, ref, "dW %dx%d" % (cin, cout))


@pytest.mark.parametrize("shape,cin,cout", [CASES[1], CASES[5]], ids=[IDS[1], IDS[5]])
def test_conv_dw_segments_accumulate(shape, cin, cout):
    init = torch.randn(cout, 5 * cin, generator=torch.Generator().manual_seed(3))
    got, ref = run(shape, cin, cout, init=init)
    check(got, ref + init.double().reshape(cout, cin, 5), "dW += %dx%d" % (cin, cout))


def test_conv_dw_segments_without_lengths():
    got, ref = run(SHAPE_B, 32, 32, masked=False)
    check(got, ref, "dW, every utterance T rows")


def test_postnet_backward_bf16_ragged_against_oracle():
    from test_gpu_model import build
    B, T, lens = SHAPE_A
    m, cfg, st, hp = build(TINY, compute_dtype="bf16")
    assert cfg.num_mels % 8 == 0 and cfg.postnet_hidden % 8 == 0          # (the segmented path, not the gather fall-back)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, T, cfg.num_mels, generator=g)
    go = torch.randn(B, T, cfg.num_mels, generator=g)
    ln = torch.tensor(lens)
    P = O.to_torch_state(st)
    names = ["postnet.conv_layers.%d.weight" % i for i in range(cfg.n_postnet_layer)]
    for n in names:
        P[n] = P[n].detach().clone().requires_grad_(True)
    O.postnet_forward(P, cfg, x, ln, train=True).backward(go)
    post = m.postnet
    post.train()
    out = post(x.to(DEV), ln.to(DEV))
    out.backward(go.to(DEV))
    torch.cuda.synchronize()
    worst = 0.0
    for i, n in enumerate(names):
        got, ref = post.conv_layers[i].weight.grad.detach().cpu().double(), P[n].grad.double()
        rel = abs(float(got.norm()) - float(ref.norm())) / float(ref.norm())
        cos = float((got * ref).sum() / (got.norm() * ref.norm()))
        print("%s: |got| = %.4e |ref| = %.4e rel = %.4f cos = %.5f" % (n, float(got.norm()), float(ref.norm()), rel, cos))
        worst = max(worst, rel)
        # a wrong tap / channel placement keeps the norm: the direction must agree as well (bf16 operands: 1 - cos ~ 1e-4)
        assert cos > 0.99, (n, cos)
    assert worst < drift_gate("tiny96/worst_grad_norm_rel", 0.06, floor=0.02), worst
