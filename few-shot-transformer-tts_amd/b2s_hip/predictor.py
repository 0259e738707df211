"""ctypes binding of libb2s_vp.so (C ABI in include/b2s_vp.h): the variance predictors of a FastSpeech-2-style student on the GPU,
forward and backward.

b2s_hip.variance consumes a duration, a pitch and an energy per input unit; this module predicts them from the encoder output
(DESIGN.md section p): Conv1d(k=3) -> ReLU -> LayerNorm -> Dropout, the same again, then Linear to one scalar per position.  All of
it is fp32 with every rounding placed by the definition, so the results repeat bit for bit, for an utterance alone or inside a
batch, and the gradients are exact sums in a fixed order without atomics.  There is no CPU fallback.

    dp = VariancePredictor(768).cuda()
    out = dp(encoder_output, input_lengths, seed=step)            # {"prediction": [B, S], "status": [B]}
    loss = masked_mse(out["prediction"], torch.log1p(durations))  # the loss stays the caller's
    # synthesis: no targets
    dur = durations_from_prediction(dp.eval()(encoder_output, input_lengths)["prediction"], input_lengths)
    frames = variance.expand(encoder_output, dur, input_lengths)
"""
import ctypes as C

import torch

from . import ragged
from .cbind import EMPTY, FAILED, OK  # noqa: F401 (the status words are part of this module's surface)
from .cbind import B2SError, Library, dptr, nptr, raise_failed, stream
from .ragged import lengths_i32

STATUS_NAMES = ("OK", "EMPTY", "FAILED")
MAX_S, MAX_D = 1024, 1024
FILTERS = (64, 128, 256, 512)
PARAM_NAMES = ("W1", "b1", "g1", "be1", "W2", "b2", "g2", "be2", "wl", "bl")
DEFAULT_MAX_FRAMES = 1024              # per position: MAX_S positions of it stay inside variance.MAX_FRAMES per utterance

P = C.c_void_p
_I = C.c_int
_PROTOS = {
    "b2s_vp_version": (C.c_int, []),
    "b2s_vp_last_error": (C.c_char_p, []),
    "b2s_vp_ws_bytes": (C.c_size_t, [_I, _I, _I, _I]),
    "b2s_vp_tape_bytes": (C.c_size_t, [_I, _I, _I]),
    "b2s_vp_forward": (C.c_int, [P] * 12 + [C.c_float, C.c_double, C.c_uint64, _I, _I, _I, _I, P, P, P, P, C.c_size_t, P]),
    "b2s_vp_backward": (C.c_int, [P] * 14 + [C.c_double, C.c_uint64, _I, _I, _I, _I] + [P] * 12 + [C.c_size_t, P]),
    "b2s_vp_dropout_mask": (C.c_int, [C.c_double, C.c_uint64, _I, _I, _I, _I, P, P]),
}
_LIB = Library("libb2s_vp.so", _PROTOS, "b2s_vp_last_error")
LIB_PATH, EXPORTS, load, check, workspace = _LIB.path, _LIB.exports, _LIB.load, _LIB.check, _LIB.workspace


def _seed(seed):
    return int(seed) & 0xFFFFFFFFFFFFFFFF


class _Predict(torch.autograd.Function):
    """b2s_vp_forward, and b2s_vp_backward as its backward.  x and the parameters are fp32 on one GPU; n_in is device int32."""

    @staticmethod
    def forward(ctx, x, n_in, p, seed, eps, *params):
        lib = load()
        device = x.device
        B, S, D = (int(v) for v in x.shape)
        F = int(params[0].shape[0])
        x = x.contiguous()
        params = tuple(t.contiguous() for t in params)
        taped = any(ctx.needs_input_grad)
        ws_n = lib.b2s_vp_ws_bytes(B, S, D, F)
        ws = workspace(ws_n, device)
        tape = workspace(lib.b2s_vp_tape_bytes(B, S, F), device) if taped else None
        pred = torch.zeros(B, S, dtype=torch.float32, device=device)      # the rows of a FAILED utterance are not written
        status = torch.empty(B, dtype=torch.int32, device=device)
        with torch.cuda.device(device):
            check(lib.b2s_vp_forward(nptr(x), nptr(n_in), *[nptr(t) for t in params], float(eps), float(p), _seed(seed), B, S, D, F,
                                     nptr(pred), nptr(status), dptr(tape), dptr(ws), ws_n, stream(device)))
        if taped:
            ctx.save_for_backward(x, n_in, tape, *params)
        ctx.call = (B, S, D, F, float(p), _seed(seed), ws_n)
        ctx.mark_non_differentiable(status)
        return pred, status

    @staticmethod
    def backward(ctx, d_pred, _dstatus):
        lib = load()
        x, n_in, tape = ctx.saved_tensors[:3]
        params = ctx.saved_tensors[3:]
        B, S, D, F, p, seed, ws_n = ctx.call
        device = x.device
        d_pred = d_pred.to(torch.float32).contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        grads = [torch.empty_like(t) for t in params] if any(ctx.needs_input_grad[5:]) else [None] * 10
        ws = workspace(ws_n, device)
        with torch.cuda.device(device):
            check(lib.b2s_vp_backward(nptr(x), nptr(n_in), *[nptr(t) for t in params], dptr(tape), nptr(d_pred), p, seed, B, S, D, F,
                                      dptr(dx), *[dptr(g) for g in grads], dptr(ws), ws_n, stream(device)))
        return (dx, None, None, None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[5:]))


def _check_params(params, D, device):
    if isinstance(params, dict):
        params = [params[k] for k in PARAM_NAMES]
    params = list(params)
    if len(params) != 10:
        raise B2SError("the predictor has 10 parameters %s (got %d)" % (PARAM_NAMES, len(params)))
    F = int(params[0].shape[0])
    if F not in FILTERS:
        raise B2SError("F must be 64, 128, 256 or 512 (got %d)" % F)
    shapes = [(F, D, 3), (F,), (F,), (F,), (F, F, 3), (F,), (F,), (F,), (F,), (1,)]
    for name, t, shape in zip(PARAM_NAMES, params, shapes):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != device:
            raise B2SError("%s must be an fp32 tensor on %s" % (name, device))
        if int(t.numel()) != int(torch.Size(shape).numel()) or (t.dim() == 3 and tuple(t.shape) != shape):
            raise B2SError("%s must have the shape %s (got %s)" % (name, shape, tuple(t.shape)))
    return params


def predict(x, input_lengths, params, p=0.0, seed=0, check_status=True, eps=1e-5):
    """x [B, S, D] fp32 on the GPU, input_lengths [B]; params: the ten tensors W1 [F, D, 3], b1, g1, be1 [F], W2 [F, F, 3], b2, g2,
    be2 [F], wl [F] (or [1, F]), bl [1] in that order, or a dict by those names.  p in [0, 1) with seed: the dropout behind both
    LayerNorms.  Differentiable in x and every parameter (b2s_vp_backward).

    Returns (prediction [B, S] fp32, zeros from input_lengths on and for a FAILED utterance; status [B] int32).  check_status reads
    the status words and raises B2SError for a FAILED utterance; False leaves the words to the caller and reads nothing."""
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.dtype != torch.float32 or not x.is_cuda:
        raise B2SError("x must be an fp32 tensor [B, S, D] on the GPU")
    device = ragged.device("the variance predictor", x)
    B, S, D = (int(v) for v in x.shape)
    if not 0.0 <= float(p) < 1.0:
        raise B2SError("p must be in [0, 1) (got %r)" % (p,))
    params = _check_params(params, D, device)
    n_in = lengths_i32(input_lengths, B, device, "input_lengths")
    pred, status = _Predict.apply(x, n_in, float(p), int(seed), float(eps), *params)
    if check_status:
        raise_failed(status, "the variance predictor", "utterances", "a length outside 0..S")
    return pred, status


def dropout_mask(p, seed, site, B, S, F, device=None):
    """b2s_vp_dropout_mask: the keep bytes [B, S, F] (uint8) of the dropout at `site` (1 or 2)."""
    lib = load()
    device = ragged.device("the variance predictor") if device is None else torch.device(device)
    out = torch.empty(max(B, 0), max(S, 0), max(F, 0), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        check(lib.b2s_vp_dropout_mask(float(p), _seed(seed), int(site), B, S, F, nptr(out), stream(device)))
    return out


def durations_from_prediction(pred, input_lengths, alpha=1.0, max_frames=DEFAULT_MAX_FRAMES):
    """Frames per position from a duration prediction in the log domain: clamp(round((exp(pred) - 1) * alpha), 0, max_frames) as
    int32 [B, S], zero from input_lengths on; what variance.expand takes as durations.  torch ops in fp64 where pred is; nothing is
    copied to the host."""
    if pred.dim() != 2:
        raise B2SError("pred must be [B, S], got %s" % (tuple(pred.shape),))
    B, S = (int(v) for v in pred.shape)
    n = lengths_i32(input_lengths, B, pred.device, "input_lengths")
    d = torch.clamp(torch.round((torch.exp(pred.detach().to(torch.float64)) - 1.0) * float(alpha)), 0, int(max_frames)).to(torch.int32)
    valid = torch.arange(S, device=pred.device).unsqueeze(0) < n.unsqueeze(1)
    return d * valid.to(torch.int32)


class VariancePredictor(torch.nn.Module):
    """One variance predictor (duration, pitch or energy).  The parameters live in the submodules conv1, norm1, conv2, norm2 and
    linear, so a state_dict is that of the plain torch composition (reference_forward)."""

    def __init__(self, dim, filter_size=256, dropout=0.5, eps=1e-5):
        super(VariancePredictor, self).__init__()
        if dim < 4 or dim > MAX_D or dim % 4:
            raise B2SError("D must be a multiple of 4 in 4..%d (got %d)" % (MAX_D, dim))
        if filter_size not in FILTERS:
            raise B2SError("F must be 64, 128, 256 or 512 (got %d)" % filter_size)
        if not 0.0 <= dropout < 1.0:
            raise B2SError("p must be in [0, 1) (got %r)" % (dropout,))
        self.dim, self.filter_size, self.dropout, self.eps = int(dim), int(filter_size), float(dropout), float(eps)
        self.conv1 = torch.nn.Conv1d(dim, filter_size, 3, padding=1)
        self.norm1 = torch.nn.LayerNorm(filter_size, eps=eps)
        self.conv2 = torch.nn.Conv1d(filter_size, filter_size, 3, padding=1)
        self.norm2 = torch.nn.LayerNorm(filter_size, eps=eps)
        self.linear = torch.nn.Linear(filter_size, 1)

    def parameters_in_order(self):
        return [self.conv1.weight, self.conv1.bias, self.norm1.weight, self.norm1.bias, self.conv2.weight, self.conv2.bias,
                self.norm2.weight, self.norm2.bias, self.linear.weight, self.linear.bias]

    def forward(self, x, input_lengths, seed=0, check_status=True):
        """x [B, S, D], input_lengths [B] -> {"prediction": [B, S], "status": [B]}.  Dropout is live only in train(), where `seed`
        picks the mask (pass the step number); eval() ignores it."""
        p = self.dropout if self.training else 0.0
        pred, status = predict(x, input_lengths, self.parameters_in_order(), p=p, seed=seed if self.training else 0,
                               check_status=check_status, eps=self.eps)
        return {"prediction": pred, "status": status}

    def reference_forward(self, x, input_lengths, keep=None):
        """The plain torch composition of the same submodules, on any device and in the parameters' dtype: the baseline of the
        benchmark and the host tests.  keep: None (torch's own dropout in train()) or the two keep masks [B, S, F] to apply with the
        scale 1 / (1 - p).  Lengths must be in 0..S."""
        B, S, _ = x.shape
        n = torch.as_tensor(input_lengths, device=x.device).reshape(-1)
        valid = (torch.arange(S, device=x.device).unsqueeze(0) < n.unsqueeze(1)).to(x.dtype).unsqueeze(-1)
        h = x * valid
        for i, (conv, norm) in enumerate(((self.conv1, self.norm1), (self.conv2, self.norm2))):
            h = norm(torch.relu(conv(h.transpose(1, 2)).transpose(1, 2)))
            if keep is not None:
                h = h * keep[i].to(h.dtype) * (1.0 / (1.0 - self.dropout))
            else:
                h = torch.nn.functional.dropout(h, self.dropout, self.training)
            h = h * valid
        return self.linear(h).squeeze(-1) * valid.squeeze(-1)
