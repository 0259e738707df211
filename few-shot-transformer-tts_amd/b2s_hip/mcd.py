"""ctypes binding of libb2s_mcd.so (C ABI in include/b2s_mcd.h): mel-cepstral distortion after DTW (MCD-DTW, in dB) on the GPU.

The objective score that TTS papers report, from the two things a finished eval already has: the generated mels and the ground
truth of mels.zip.  Per pair (DESIGN.md section k): voiced frames of each side (the reference's rule in calculate_mse_dtw: max over
the bins > 0), normalised mel -> natural-log magnitude in fp64, rows 1..order of the orthonormal DCT-II over the mel bins (c_0, the
energy, is not used), fp32 cepstra, the batched FastDTW of b2s_hip.metrics on them (euclidean, radius 1 by default, radius=None the
exact dtw), then the mean over the path of 10 / ln 10 * sqrt(2 * sum_k (cx_k - cy_k)^2).  Bit-reproducible, and the same bits for a
pair alone or inside a batch.  There is no CPU fallback: a missing library is an error.

    python -m b2s_hip.mcd EVAL_DIR --data-dir DATA_DIR [--zipfilepath Z] [--eval-meta M] [--order 13] [--radius 1|exact]
                          [--batch 64] [--json OUT]

re-scores a finished eval: every EVAL_DIR/<name>.npy against member <name>.npy of mels.zip.
"""
import ctypes as C
import math
import sys

import numpy as np
import torch

from . import metrics, ragged, rescore
from .cbind import EMPTY, FAILED, OK, B2SError, Library, default_hp, nptr, raise_failed, stream

MAX_MELS, MAX_ORDER = 512, 256
LN_SCALE = math.log(10.0) / 20.0           # dB -> natural-log magnitude
DB_SCALE = 10.0 / math.log(10.0)           # the MCD's 10 / ln 10

P = C.c_void_p
_I = C.c_int
_D = C.c_double
_PROTOS = {
    "b2s_mcd_version": (C.c_int, []),
    "b2s_mcd_last_error": (C.c_char_p, []),
    "b2s_mcd_ws_bytes": (C.c_size_t, [_I, _I]),
    "b2s_mcd_cepstra": (C.c_int, [P, P, _I, _I, _I, _I, _I, P, _I, _D, _D, _D, _D, P, P, P, P, P, C.c_size_t, P]),
    "b2s_mcd_score": (C.c_int, [P, P, _I, P, P, _I, _I, _I, P, P, _I, P, P, _D, P, P, P, P]),
}
_LIB = Library("libb2s_mcd.so", _PROTOS, "b2s_mcd_last_error")
LIB_PATH, EXPORTS, load, check, workspace = _LIB.path, _LIB.exports, _LIB.load, _LIB.check, _LIB.workspace


def dct_table(n_mels, order):
    """Rows 1..order of the orthonormal DCT-II over n_mels bins, float64 [order, n_mels]:
    D[k, m] = sqrt(2 / n_mels) * cos(pi / n_mels * (m + 0.5) * k).  Computed once here and handed to the kernel as data."""
    n_mels, order = int(n_mels), int(order)
    if not 2 <= n_mels <= MAX_MELS:
        raise B2SError("n_mels must be in 2..%d (got %d)" % (MAX_MELS, n_mels))
    if not 1 <= order <= min(n_mels - 1, MAX_ORDER):
        raise B2SError("order must be in 1..%d for %d mel bins (got %d)" % (min(n_mels - 1, MAX_ORDER), n_mels, order))
    k = np.arange(1, order + 1, dtype=np.float64)[:, None]
    m = np.arange(n_mels, dtype=np.float64)[None, :]
    return np.sqrt(2.0 / n_mels) * np.cos(np.pi / n_mels * (m + 0.5) * k)


_tables = {}


def _device_table(n_mels, order, device):
    key = (n_mels, order, str(device))
    if key not in _tables:
        _tables[key] = torch.from_numpy(dct_table(n_mels, order)).to(device)
    return _tables[key]


def cepstra_packed(rows, offsets, max_len, order=13, hp=None):
    """b2s_mcd_cepstra on packed device rows [total, n_mels] fp32 with their B + 1 int32 device offsets; max_len bounds every length.
    No host read.  Returns device tensors: cep (a buffer of `total` rows of which the first offsets[B] are written), offsets
    [B + 1], voiced [B] and status [B]."""
    lib = load()
    hp = default_hp(hp)
    device = rows.device
    total, n_mels = int(rows.shape[0]), int(rows.shape[1])
    B = int(offsets.numel()) - 1
    order = int(order)
    table = _device_table(n_mels, order, device)               # refuses a bad n_mels / order
    nbytes = lib.b2s_mcd_ws_bytes(B, int(max_len))
    ws = workspace(nbytes, device)
    cep = torch.empty(total, order, dtype=torch.float32, device=device)
    off = torch.empty(B + 1, dtype=torch.int32, device=device)
    voiced = torch.empty(B, dtype=torch.int32, device=device)
    status = torch.empty(B, dtype=torch.int32, device=device)
    check(lib.b2s_mcd_cepstra(nptr(rows), nptr(offsets), total, int(max_len), B, n_mels, order, nptr(table),
                              1 if hp.symmetric_mel else 0, float(hp.max_abs_value), float(hp.max_db), float(hp.ref_db), LN_SCALE,
                              nptr(cep), nptr(off), nptr(voiced), nptr(status), nptr(ws), nbytes, stream(device)))
    return {"cep": cep, "offsets": off, "voiced": voiced, "status": status}


def score_packed(cep_x, offsets_x, total_x, cep_y, offsets_y, total_y, path, path_offsets, path_len, dtw_status):
    """b2s_mcd_score on what cepstra_packed and b2s_met_dtw left on the device: the two cepstral buffers with their B + 1 offsets
    and host totals, path [total_path, 2] int32 with its B + 1 device offsets, path_len [B] and the DTW's status [B].  No host read.
    Returns device tensors: mcd [B] f64, status [B] int32 and dist [total_path] f64 (NaN where no step was written)."""
    lib = load()
    device = cep_x.device
    B, order, tp = int(path_len.numel()), int(cep_x.shape[1]), int(path.shape[0])
    mcd = torch.empty(B, dtype=torch.float64, device=device)
    status = torch.empty(B, dtype=torch.int32, device=device)
    dist = torch.full((tp,), float("nan"), dtype=torch.float64, device=device)
    check(lib.b2s_mcd_score(nptr(cep_x), nptr(offsets_x), int(total_x), nptr(cep_y), nptr(offsets_y), int(total_y), B, order,
                            nptr(path), nptr(path_offsets), tp, nptr(path_len), nptr(dtw_status), DB_SCALE, nptr(mcd), nptr(status),
                            nptr(dist), stream(device)))
    return mcd, status, dist


def pack_batch(mels, lengths, device=None, what="mels"):
    """Padded [B, T, n_mels] NumPy array or tensor on any device -> (packed fp32 device rows [sum(lengths), n_mels], their B + 1
    int32 device offsets, the longest length): what cepstra_packed takes."""
    t = ragged.as_batch(mels, _pick_device(mels) if device is None else device, what)
    if int(t.shape[0]) == 0:
        raise B2SError("%s holds no utterance" % what)
    n = ragged.lengths(lengths, int(t.shape[0]), int(t.shape[1]), what + "_lengths")
    rows, off = ragged.pack(t, n)
    return rows, torch.from_numpy(off).to(t.device), max(n)


def _pick_device(*arrays):
    return ragged.device("the DTW metric", *arrays)


def cepstra_batch(mels, lengths, order=13, hp=None):
    """Voiced frames of every utterance as mel cepstra c_1..c_order.  mels: padded [B, T, n_mels] NumPy array or tensor on any device
    (normalised mel scale), lengths [B].  Returns device tensors: the cepstra of the whole batch packed gap-free [total_voiced,
    order] fp32, their B + 1 int32 offsets, and the voiced counts [B] int32.  One host read (offsets and status) sizes the result."""
    rows, off_d, max_len = pack_batch(mels, lengths)
    out = cepstra_packed(rows, off_d, max_len, order, hp)
    host = torch.cat([out["offsets"], out["status"]]).cpu().numpy()
    B = len(host) // 2
    raise_failed(host[B + 1:], "cepstra", "utterances")
    return out["cep"][:int(host[B])], out["offsets"], out["voiced"]


def mcd_dtw_details(preds, pred_lengths, targets, target_lengths, order=13, radius=1, hp=None):
    """Everything one scoring call produces, as a dict of device tensors (host where noted): mcd [B] f64 (NaN unless status is OK),
    status [B] int32 (OK / EMPTY / FAILED, nothing raised here), voiced_x / voiced_y [B], path_len [B], path [sum, 2] int32 with the
    host array path_offsets [B + 1], dist [sum] f64 (the per-step distortion in dB, laid out like the path), cep_x / cep_y with
    offsets_x / offsets_y.  The two B + 1 voiced-offset arrays are read back once in the middle of the call (the DTW entry point takes
    its totals and maxima from the host); everything else is queued on the current stream."""
    device = _pick_device(preds, targets)
    xr, xo_d, mx = pack_batch(preds, pred_lengths, device, "preds")
    yr, yo_d, my = pack_batch(targets, target_lengths, device, "targets")
    B, By = int(xo_d.numel()) - 1, int(yo_d.numel()) - 1
    if B != By:
        raise B2SError("preds has %d utterances, targets has %d" % (B, By))
    if int(xr.shape[1]) != int(yr.shape[1]):
        raise B2SError("preds has %d mel bins, targets has %d" % (int(xr.shape[1]), int(yr.shape[1])))
    r = metrics.c_radius(radius)
    order = int(order)
    cx = cepstra_packed(xr, xo_d, mx, order, hp)
    cy = cepstra_packed(yr, yo_d, my, order, hp)
    host = torch.stack([cx["offsets"], cy["offsets"]]).cpu().numpy()           # the one host read in front of the DTW
    vx, vy = np.diff(host[0]), np.diff(host[1])
    tx, ty, vmx, vmy = int(host[0, -1]), int(host[1, -1]), int(vx.max()), int(vy.max())
    dtw = metrics.dtw_packed(cx["cep"], cx["offsets"], tx, vmx, cy["cep"], cy["offsets"], ty, vmy, B, order, r, 0,
                             ragged.offsets(vx + vy))
    path, po, po_d, plen, dstat = dtw["path"], dtw["path_offsets"], dtw["path_offsets_device"], dtw["path_len"], dtw["status"]
    mcd, sstat, dist = score_packed(cx["cep"], cx["offsets"], tx, cy["cep"], cy["offsets"], ty, path, po_d, plen, dstat)
    failed = (cx["status"] == FAILED) | (cy["status"] == FAILED)
    status = torch.where(failed, torch.full_like(sstat, FAILED), sstat)
    mcd = torch.where(status == OK, mcd, torch.full_like(mcd, float("nan")))
    return {"mcd": mcd, "status": status, "voiced_x": cx["voiced"], "voiced_y": cy["voiced"], "path_len": plen, "path": path,
            "path_offsets": po, "path_offsets_device": po_d, "dtw_status": dstat, "dist": dist, "dtw_cost": dtw["cost"], "cep_x": cx["cep"][:tx], "cep_y": cy["cep"][:ty],
            "offsets_x": cx["offsets"], "offsets_y": cy["offsets"]}


def mcd_dtw_batch(preds, pred_lengths, targets, target_lengths, order=13, radius=1, hp=None, return_paths=False):
    """MCD-DTW in dB of every pair, as a float64 device tensor [B]; NaN where a side has no voiced frame (status EMPTY).  preds,
    targets: padded [B, T, n_mels] NumPy arrays or tensors on any device, in the normalised mel scale of `hp` (default: the global
    hyper-parameters).  radius >= 1 is fastdtw's radius, None the exact dtw.  With return_paths also the list of int64 [L_b, 2] host
    paths over the voiced frames.  Raises B2SError when a pair FAILED.  Two host reads: the two B + 1 voiced-offset arrays in front of
    the DTW (it needs host totals and maxima) and, because a FAILED pair has to raise, the B status words at the end.  An empty batch
    gives an empty tensor."""
    if len(preds) == 0:
        empty = torch.empty(0, dtype=torch.float64, device=_pick_device(preds, targets))
        return (empty, []) if return_paths else empty
    out = mcd_dtw_details(preds, pred_lengths, targets, target_lengths, order=order, radius=radius, hp=hp)
    raise_failed(out["status"], "MCD after DTW", "utterances")
    return (out["mcd"], ragged.paths(out)) if return_paths else out["mcd"]


def calculate_mcd_dtw(preds, pred_lengths, targets, target_lengths, order=13, radius=1, hp=None):
    """The list shape of calculate_mse_dtw: one Python float (dB) per pair, None where a side has no voiced frame."""
    if len(preds) == 0:
        return []
    m = mcd_dtw_batch(preds, pred_lengths, targets, target_lengths, order=order, radius=radius, hp=hp).cpu().numpy()
    return [None if np.isnan(v) else float(v) for v in m]


# ------------------------------------------------------------------------------------------------------- re-scoring a finished eval

def score_eval_dir(eval_dir, zipfilepath, eval_meta=None, order=13, radius=1, batch=64, hp=None):
    """Score every `<name>.npy` of eval_dir against member `<name>.npy` of the mels.zip, `batch` pairs per GPU call (only one
    batch of mels is in memory at a time).  Returns the summary dict: overall and per-language mean MCD over the scored records, the
    counts (scored, empty, without a target) and the per-record scores."""
    hp = default_hp(hp)
    lang = rescore.languages(eval_meta, hp)
    records = []

    def score(part, preds, pl, targets, tl):
        out = mcd_dtw_details(preds, pl, targets, tl, order=order, radius=radius, hp=hp)
        host = {k: out[k].cpu().numpy() for k in ("mcd", "status", "voiced_x", "voiced_y", "path_len")}
        raise_failed(host["status"], "MCD after DTW", "utterances")
        for j, n in enumerate(part):
            empty = int(host["status"][j]) == EMPTY
            records.append({"name": n, "language": lang.get(n), "mcd": None if empty else float(host["mcd"][j]),
                            "voiced_pred": int(host["voiced_x"][j]), "voiced_target": int(host["voiced_y"][j]),
                            "path_len": int(host["path_len"][j])})
    no_target = rescore.walk(eval_dir, zipfilepath, batch, score)
    head = {"metric": "mcd_dtw_db", "order": int(order), "radius": "exact" if radius is None else int(radius)}
    return rescore.summary(head, records, [r for r in records if r["mcd"] is not None], no_target, ("mcd",))


@rescore.cli
def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m b2s_hip.mcd", description="Re-score a finished eval with MCD-DTW on the GPU.")
    rescore.add_arguments(ap, "eval_dir", "--data-dir", "--zipfilepath", "--eval-meta")
    ap.add_argument("--order", type=int, default=13, help="cepstral coefficients c_1..c_order")
    rescore.add_arguments(ap, "--radius", "--batch", "--json")
    a = ap.parse_args(argv)
    zipfilepath, eval_meta = rescore.inputs(a)
    radius = rescore.radius(a.radius)
    from hyperparams import hparams as hp
    top = min(int(hp.num_mels) - 1, MAX_ORDER)
    if not 1 <= a.order <= top:
        raise rescore.UsageError("--order must be in 1..%d for %d mel bins (got %d)" % (top, int(hp.num_mels), a.order))
    rescore.batch(a.batch)
    rescore.found("EVAL_DIR", a.eval_dir, isdir=True)
    rescore.found("mels.zip", zipfilepath)
    res = score_eval_dir(a.eval_dir, zipfilepath, eval_meta, order=a.order, radius=radius, batch=a.batch, hp=hp)
    return rescore.finish(res, a.json, ("records", "without_target"))


if __name__ == "__main__":
    sys.exit(main())
