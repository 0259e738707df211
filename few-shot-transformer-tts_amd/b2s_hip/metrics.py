"""ctypes binding of libb2s_metrics.so (C ABI in include/b2s_metrics.h): batched FastDTW and the MSE-after-DTW eval metric on the GPU.

fastdtw 0.3.4's fastdtw(x, y, radius, dist=euclidean) (radius >= 1) and dtw(x, y) (radius=None here, -1 in the C ABI), batched over
ragged pairs, fp64 distances and costs; the paths are those of the library.  calculate_mse_dtw has the reference's signature
(utils/infolog.py) and takes NumPy arrays or torch tensors on any device.  There is no CPU fallback: a missing library is an error.

install(hp) puts calculate_mse_dtw in place of the reference's utils.infolog.calculate_mse_dtw when hp.mse_dtw == "hip" (and
restores the original for "reference"); synthesize.eval_batch calls it, so the unedited eval.py picks the GPU metric up.
"""
import ctypes as C
import logging

import numpy as np
import torch

from . import ragged
from .cbind import EMPTY, FAILED, OK  # noqa: F401 (the status words are part of this module's surface)
from .cbind import B2SError, Library, choice, nptr, raise_failed, rebind, stream

VOICED_ONLY = 1

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
_LIB = Library("libb2s_metrics.so", _PROTOS, "b2s_met_last_error")
LIB_PATH, EXPORTS, load, check, workspace = _LIB.path, _LIB.exports, _LIB.load, _LIB.check, _LIB.workspace


def c_radius(radius):
    """fastdtw's radius as the C ABI takes it: >= 1, or -1 for None (the exact dtw)."""
    if radius is None:
        return -1
    radius = int(radius)
    if radius < 1:
        raise B2SError("radius must be >= 1, or None for the exact dtw (got %d)" % radius)
    return radius


def dtw_packed(xp, xo_d, tx, mx, yp, yo_d, ty, my, B, dim, r, flags, path_offsets=None):
    """One b2s_met_dtw call on packed device rows xp [tx, dim] / yp [ty, dim] fp32 with their B + 1 int32 device offsets, the host
    totals tx / ty and longest lengths mx / my; r from c_radius.  `path_offsets` (B + 1 int32 on the host, each pair's room at least
    its two lengths summed) asks for the paths.  No host read; queued on the current stream.  Returns device tensors: cost and mse
    [B] f64, path_len and status [B] int32, and with path_offsets also path [total, 2] int32, path_offsets_device and path_offsets
    itself (the host array)."""
    lib = load()
    device = xo_d.device
    nbytes = lib.b2s_met_dtw_ws_bytes(B, tx, ty, mx, my, dim, r, flags)
    ws = workspace(nbytes, device)
    out = {"cost": torch.empty(B, dtype=torch.float64, device=device), "mse": torch.empty(B, dtype=torch.float64, device=device),
           "path_len": torch.empty(B, dtype=torch.int32, device=device), "status": torch.empty(B, dtype=torch.int32, device=device)}
    path = po_d = None
    if path_offsets is not None:
        path = out["path"] = torch.empty(max(1, int(path_offsets[-1])), 2, dtype=torch.int32, device=device)
        po_d = out["path_offsets_device"] = torch.from_numpy(path_offsets).to(device)
        out["path_offsets"] = path_offsets
    check(lib.b2s_met_dtw(nptr(xp), nptr(xo_d), tx, mx, nptr(yp), nptr(yo_d), ty, my, B, dim, r, flags, nptr(out["cost"]),
                          nptr(out["mse"]), nptr(out["path_len"]), nptr(out["status"]), nptr(path), nptr(po_d), nptr(ws), nbytes,
                          stream(device)))
    return out


def _run(x, x_lengths, y, y_lengths, radius, flags, return_paths):
    device = ragged.device("the DTW metric", x)
    xt, yt = ragged.as_batch(x, device, "x"), ragged.as_batch(y, device, "y")
    B = int(xt.shape[0])
    if int(yt.shape[0]) != B:
        raise B2SError("x has %d pairs, y has %d" % (B, int(yt.shape[0])))
    dim = int(xt.shape[2])
    if int(yt.shape[2]) != dim:
        raise B2SError("x has %d features, y has %d" % (dim, int(yt.shape[2])))
    lx = ragged.lengths(x_lengths, B, int(xt.shape[1]), "x_lengths")
    ly = ragged.lengths(y_lengths, B, int(yt.shape[1]), "y_lengths")
    r = c_radius(radius)
    xp, xo = ragged.pack(xt, lx)
    yp, yo = ragged.pack(yt, ly)
    po = ragged.offsets([a + b for a, b in zip(lx, ly)]) if return_paths else None
    return dtw_packed(xp, torch.from_numpy(xo).to(device), int(xo[-1]), max(lx), yp, torch.from_numpy(yo).to(device), int(yo[-1]),
                      max(ly), B, dim, r, flags, po)


def dtw_batch(x, x_lengths, y, y_lengths, radius=1, return_paths=False):
    """fastdtw(x_b[:lx_b], y_b[:ly_b], radius) with euclidean distance for every pair (radius=None: the exact dtw), all frames kept.
    x, y: padded [B, T, dim] (or [B, T]) NumPy arrays or tensors on any device.  Returns the costs as a float64 device tensor [B]
    (NaN where a side is empty), and with return_paths also the list of int64 [L_b, 2] host paths."""
    out = _run(x, x_lengths, y, y_lengths, radius, 0, return_paths)
    raise_failed(out["status"], "DTW")
    cost = torch.where(out["status"] == OK, out["cost"], torch.full_like(out["cost"], float("nan")))
    return (cost, ragged.paths(out)) if return_paths else cost


def fastdtw(x, y, radius=1):
    """One pair, fastdtw's return value: (distance, [(i, j), ...]).  x, y: [T, dim] or [T]."""
    x, y = ragged.as_tensor(x), ragged.as_tensor(y)
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
    on = choice(hp, "mse_dtw") == "hip"
    if rebind("utils.infolog", "calculate_mse_dtw", calculate_mse_dtw, _ORIGINAL, on):
        logging.info("mse_dtw=hip: utils.infolog.calculate_mse_dtw now runs on the GPU (b2s_hip.metrics)" if on else
                     "mse_dtw=reference: utils.infolog.calculate_mse_dtw restored")
