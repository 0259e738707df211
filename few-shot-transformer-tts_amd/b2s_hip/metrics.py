"""ctypes binding of libb2s_metrics.so (C ABI in include/b2s_metrics.h): batched FastDTW and the MSE-after-DTW eval metric on the GPU.

fastdtw 0.3.4's fastdtw(x, y, radius, dist=euclidean) (radius >= 1) and dtw(x, y) (radius=None here, -1 in the C ABI), batched over
ragged pairs, fp64 distances and costs; the paths are those of the library.  calculate_mse_dtw has the reference's signature
(utils/infolog.py) and takes NumPy arrays or torch tensors on any device.  There is no CPU fallback: a missing library is an error.

install(hp) puts calculate_mse_dtw in place of the reference's utils.infolog.calculate_mse_dtw when hp.mse_dtw == "hip" (and
restores the original for "reference"); synthesize.eval_batch calls it, so the unedited eval.py picks the GPU metric up.
"""
import ctypes as C
import logging
import os
import sys

import numpy as np
import torch

from .lib import B2SError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "libb2s_metrics.so")

VOICED_ONLY = 1
OK, EMPTY, FAILED = 0, 1, 2
MSE_DTW_CHOICES = ("reference", "hip")

P = C.c_void_p
_I = C.c_int
_PROTOS = {
    "b2s_met_version": (C.c_int, []),
    "b2s_met_last_error": (C.c_char_p, []),
    "b2s_met_dtw_ws_bytes": (C.c_size_t, [_I, _I, _I, _I, _I, _I, _I, _I]),
    "b2s_met_dtw": (C.c_int, [P, P, _I, _I, P, P, _I, _I, _I, _I, _I, _I, P, P, P, P, P, P, P, C.c_size_t, P]),
    # alignment-head selection (bound in b2s_hip.alignment)
    "b2s_met_align_chunk": (C.c_int, []),
    "b2s_met_align_ws_bytes": (C.c_size_t, [_I, _I, _I, _I, _I]),
    "b2s_met_align_select": (C.c_int, [P, _I, _I, _I, _I, _I, P, P, P, P, P, P, P, P, C.c_size_t, P]),
    # batched edit distance behind the CER (bound in b2s_hip.cer)
    "b2s_met_edit_max_len": (C.c_int, []),
    "b2s_met_edit_distance": (C.c_int, [P, P, _I, _I, P, P, _I, _I, _I, P, P, P, P]),
}
EXPORTS = sorted(_PROTOS)

_lib = None


def load():
    """Load libb2s_metrics.so (raises B2SError if it is missing -- there is no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise B2SError("libb2s_metrics.so not found at %s -- build it with few-shot-transformer-tts_amd/csrc/build.sh "
                       "(or __graft_entry__.build()); there is no CPU fallback" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _PROTOS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise B2SError(load().b2s_met_last_error().decode("utf-8", "replace"))


def _c_radius(radius):
    if radius is None:
        return -1
    radius = int(radius)
    if radius < 1:
        raise B2SError("radius must be >= 1, or None for the exact dtw (got %d)" % radius)
    return radius


def _lengths(lengths, B, T, what):
    if isinstance(lengths, torch.Tensor):
        lengths = lengths.detach().cpu().numpy()
    out = [int(n) for n in np.asarray(lengths).reshape(-1)]
    if len(out) != B:
        raise B2SError("%d %s for a batch of %d" % (len(out), what, B))
    if any(n < 0 for n in out):
        raise B2SError("%s must be >= 0 (got %s)" % (what, out))
    return [min(n, T) for n in out]                    # x[i, :n] slices past the end like the reference's indexing


def _device():
    if not torch.cuda.is_available():
        raise B2SError("the DTW metric runs on the GPU only; no HIP device is visible")
    return torch.device("cuda", torch.cuda.current_device())


def _as_batch(a, device, what):
    """[B, T, dim] (or [B, T] for dim 1) NumPy array or tensor on any device -> contiguous fp32 tensor [B, T, dim] on `device`."""
    t = torch.from_numpy(np.asarray(a)) if not isinstance(a, torch.Tensor) else a.detach()
    if t.dim() == 2:
        t = t.unsqueeze(-1)
    if t.dim() != 3:
        raise B2SError("%s must be [B, T, dim] or [B, T], got %s" % (what, tuple(t.shape)))
    return t.to(device=device, dtype=torch.float32).contiguous()


def _pack(t, lengths):
    """Padded [B, T, dim] -> packed [sum(lengths), dim] rows and B + 1 int32 offsets (host and device)."""
    B, T = int(t.shape[0]), int(t.shape[1])
    mask = torch.arange(T).unsqueeze(0) < torch.tensor(lengths, dtype=torch.int64).unsqueeze(1)
    packed = t[mask.to(t.device)].contiguous()
    off = np.zeros(B + 1, dtype=np.int32)
    np.cumsum(lengths, out=off[1:])
    return packed, off


def _run(x, x_lengths, y, y_lengths, radius, flags, return_paths):
    lib = load()
    device = x.device if isinstance(x, torch.Tensor) and x.is_cuda else _device()
    xt, yt = _as_batch(x, device, "x"), _as_batch(y, device, "y")
    B = int(xt.shape[0])
    if int(yt.shape[0]) != B:
        raise B2SError("x has %d pairs, y has %d" % (B, int(yt.shape[0])))
    dim = int(xt.shape[2])
    if int(yt.shape[2]) != dim:
        raise B2SError("x has %d features, y has %d" % (dim, int(yt.shape[2])))
    lx = _lengths(x_lengths, B, int(xt.shape[1]), "x_lengths")
    ly = _lengths(y_lengths, B, int(yt.shape[1]), "y_lengths")
    r = _c_radius(radius)
    xp, xo = _pack(xt, lx)
    yp, yo = _pack(yt, ly)
    tx, ty, mx, my = int(xo[-1]), int(yo[-1]), max(lx), max(ly)
    nbytes = lib.b2s_met_dtw_ws_bytes(B, tx, ty, mx, my, dim, r, flags)
    if nbytes == 0:
        check(1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    xo_d = torch.from_numpy(xo).to(device)
    yo_d = torch.from_numpy(yo).to(device)
    cost = torch.empty(B, dtype=torch.float64, device=device)
    mse = torch.empty(B, dtype=torch.float64, device=device)
    plen = torch.empty(B, dtype=torch.int32, device=device)
    status = torch.empty(B, dtype=torch.int32, device=device)
    path = po_d = None
    if return_paths:
        po = np.zeros(B + 1, dtype=np.int32)
        np.cumsum([a + b for a, b in zip(lx, ly)], out=po[1:])
        path = torch.empty(max(1, int(po[-1])), 2, dtype=torch.int32, device=device)
        po_d = torch.from_numpy(po).to(device)

    def p(t):
        return None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())
    stream = torch.cuda.current_stream(device).cuda_stream
    check(lib.b2s_met_dtw(p(xp), p(xo_d), tx, mx, p(yp), p(yo_d), ty, my, B, dim, r, flags, p(cost), p(mse), p(plen), p(status),
                          p(path), p(po_d), p(ws), nbytes, stream))
    out = {"cost": cost, "mse": mse, "path_len": plen, "status": status}
    if return_paths:
        out["path"], out["path_offsets"] = path, po
    return out


def _paths(out):
    """Host copies of the paths: list of int64 [L_b, 2] arrays (empty for EMPTY / FAILED pairs)."""
    path = out["path"].cpu().numpy()
    plen = out["path_len"].cpu().numpy()
    po = out["path_offsets"]
    return [path[po[b]:po[b] + plen[b]].astype(np.int64) for b in range(len(plen))]


def _raise_failed(status):
    st = status.cpu().numpy()
    if np.any(st == FAILED):
        raise B2SError("DTW failed for pairs %s (offsets inconsistent with the sizes)" % np.nonzero(st == FAILED)[0].tolist())


def dtw_batch(x, x_lengths, y, y_lengths, radius=1, return_paths=False):
    """fastdtw(x_b[:lx_b], y_b[:ly_b], radius) with euclidean distance for every pair (radius=None: the exact dtw), all frames kept.
    x, y: padded [B, T, dim] (or [B, T]) NumPy arrays or tensors on any device.  Returns the costs as a float64 device tensor [B]
    (NaN where a side is empty), and with return_paths also the list of int64 [L_b, 2] host paths."""
    out = _run(x, x_lengths, y, y_lengths, radius, 0, return_paths)
    _raise_failed(out["status"])
    cost = torch.where(out["status"] == OK, out["cost"], torch.full_like(out["cost"], float("nan")))
    return (cost, _paths(out)) if return_paths else cost


def fastdtw(x, y, radius=1):
    """One pair, fastdtw's return value: (distance, [(i, j), ...]).  x, y: [T, dim] or [T]."""
    x = x if isinstance(x, torch.Tensor) else np.asarray(x)
    y = y if isinstance(y, torch.Tensor) else np.asarray(y)
    if len(x) == 0 or len(y) == 0:
        raise B2SError("fastdtw needs two non-empty sequences")
    cost, paths = dtw_batch(x[None], [len(x)], y[None], [len(y)], radius=radius, return_paths=True)
    return float(cost[0]), [(int(i), int(j)) for i, j in paths[0]]


def mse_dtw_batch(preds, pred_lengths, targets, target_lengths, radius=1):
    """The reference's MSE after DTW for every pair, as a float64 device tensor [B]: voiced frames of each side (max over the
    features > 0), fastdtw with euclidean distance, mean((x[path_x] - y[path_y])^2) over path length x features; NaN where a side
    has no voiced frame.  Runs on the current stream without synchronising."""
    out = _run(preds, pred_lengths, targets, target_lengths, radius, VOICED_ONLY, False)
    st = out["status"]
    return torch.where(st == OK, out["mse"], torch.where(st == EMPTY, torch.full_like(out["mse"], float("nan")),
                                                         torch.full_like(out["mse"], float("inf"))))


def calculate_mse_dtw(preds, pred_lengths, targets, target_lengths):
    """utils/infolog.py calculate_mse_dtw of the reference, on the GPU: a list of Python floats, None where a side has no voiced
    frame.  Accepts NumPy arrays or torch tensors on any device, lengths as lists, arrays or tensors."""
    if len(preds) == 0:
        return []
    m = mse_dtw_batch(preds, pred_lengths, targets, target_lengths).cpu().numpy()
    if np.any(np.isposinf(m)):
        raise B2SError("MSE after DTW failed for pairs %s" % np.nonzero(np.isposinf(m))[0].tolist())
    return [None if np.isnan(v) else float(v) for v in m]


# ---------------------------------------------------------------------------------------------------- opt-in for the reference eval

_ORIGINAL = "_b2s_reference_calculate_mse_dtw"


def install(hp=None):
    """Bind utils.infolog.calculate_mse_dtw (the reference's module, if imported) to this module's function for hp.mse_dtw == "hip";
    restore the original for "reference".  Anything else is a ValueError."""
    if hp is None:
        from hyperparams import hparams as hp
    mode = hp.mse_dtw
    if mode not in MSE_DTW_CHOICES:
        raise ValueError("unknown mse_dtw %r (expected 'reference' or 'hip')" % (mode,))
    mod = sys.modules.get("utils.infolog")
    if mod is None or not hasattr(mod, "calculate_mse_dtw"):
        return
    bound = mod.calculate_mse_dtw is calculate_mse_dtw
    if mode == "hip" and not bound:
        setattr(mod, _ORIGINAL, mod.calculate_mse_dtw)
        mod.calculate_mse_dtw = calculate_mse_dtw
        logging.info("mse_dtw=hip: utils.infolog.calculate_mse_dtw now runs on the GPU (b2s_hip.metrics)")
    elif mode == "reference" and bound and hasattr(mod, _ORIGINAL):
        mod.calculate_mse_dtw = getattr(mod, _ORIGINAL)
        delattr(mod, _ORIGINAL)
        logging.info("mse_dtw=reference: utils.infolog.calculate_mse_dtw restored")
