"""ctypes binding of libb2s_f0.so (C ABI in include/b2s_f0.h): batched YIN pitch tracking and the F0 error after DTW on the GPU.

The second objective score of a TTS evaluation next to MCD: does the pitch contour of the generated speech follow the target's?
Per utterance (DESIGN.md section l): the waveform becomes the int16 PCM that save_wav writes, YIN (de Cheveigne & Kawahara 2002,
steps 1 to 5) gives one F0 per frame, centred like the mel frames.  Per pair: the DTW path of b2s_hip.mcd over the kept frames (row
maximum > 0) is followed through both F0 tracks; RMSE in Hz and cents over the steps where both sides are voiced, the voicing
decision error (vde), the gross pitch error (gpe) and the F0 frame error (ffe).  Everything up to the one division per lag is an
exact integer, so the results are bit-reproducible and the same for a pair alone or inside a batch.  There is no CPU fallback.

    python -m b2s_hip.f0 EVAL_DIR --data-dir DATA_DIR [--zipfilepath Z] [--eval-meta M] [--radius 1|exact] [--batch 64] [--n-iter N]
                         [--fmin 60] [--fmax 500] [--threshold 0.1] [--silence-db -40] [--json OUT]

re-scores a finished eval: every EVAL_DIR/<name>.npy against member <name>.npy of mels.zip, both sides vocoded by mel2wav_batch.
"""
import ctypes as C
import math
import sys

import numpy as np
import torch

from . import mcd, ragged, rescore
from .cbind import EMPTY, FAILED, OK, B2SError, Library, default_hp, nptr, raise_failed, stream
from .vocoder import mel2wav_batch

MAX_WIN, MAX_TAU = 2048, 512
SCORES = ("rmse_hz", "rmse_cents", "vde", "gpe", "ffe")
COUNTS = ("steps", "vuv", "both", "gross")

P = C.c_void_p
_I = C.c_int
_D = C.c_double
_PROTOS = {
    "b2s_f0_version": (C.c_int, []),
    "b2s_f0_last_error": (C.c_char_p, []),
    "b2s_f0_quantize": (C.c_int, [P, P, _I, _I, P, P, P, P]),
    "b2s_f0_yin": (C.c_int, [P, P, P, _I, _I, _I, _I, _I, _I, _I, _D, C.c_int64, _D, P, P, P, P, P, P]),
    "b2s_f0_score": (C.c_int, [P, P, P, _I, P, P, P, _I, P, P, _I, P, P, _I, _I, P, P, _I, P, P, _D, P, P, P, P]),
}
_LIB = Library("libb2s_f0.so", _PROTOS, "b2s_f0_last_error")
LIB_PATH, EXPORTS, load, check = _LIB.path, _LIB.exports, _LIB.load, _LIB.check


def _device(*arrays):
    return ragged.device("the F0 tracker", *arrays)


def yin_params(hp=None, win=None, hop=None, tau_min=None, tau_max=None, fmin=60.0, fmax=500.0, threshold=0.1, silence_db=-40.0,
               sr=None):
    """The estimator's parameters as a dict, checked.  Defaults: win = hp.win_length, hop = hp.hop_length, tau_min = ceil(sr / fmax),
    tau_max = floor(sr / fmin), threshold 0.1, min_energy = ceil(win * (32767 * 10^(silence_db / 20))^2) (silence_db=None: 0)."""
    hp = default_hp(hp) if None in (win, hop, sr) else hp
    sr = float(hp.sr if sr is None else sr)
    win = int(hp.win_length if win is None else win)
    hop = int(hp.hop_length if hop is None else hop)
    if not sr > 0:
        raise B2SError("sr must be > 0 (got %r)" % sr)
    if not (fmin > 0 and fmax > fmin):
        raise B2SError("need 0 < fmin < fmax (got %r and %r)" % (fmin, fmax))
    tau_min = int(math.ceil(sr / fmax)) if tau_min is None else int(tau_min)
    tau_max = int(math.floor(sr / fmin)) if tau_max is None else int(tau_max)
    if not 2 <= win <= MAX_WIN:
        raise B2SError("win must be in 2..%d (got %d)" % (MAX_WIN, win))
    if hop < 1:
        raise B2SError("hop must be >= 1 (got %d)" % hop)
    if not 2 <= tau_min < tau_max <= MAX_TAU:
        raise B2SError("need 2 <= tau_min < tau_max <= %d (got %d and %d)" % (MAX_TAU, tau_min, tau_max))
    if not threshold > 0:
        raise B2SError("threshold must be > 0 (got %r)" % threshold)
    floor = 0 if silence_db is None else int(math.ceil(win * (32767.0 * 10.0 ** (float(silence_db) / 20.0)) ** 2))
    if not 0 <= floor < 2 ** 63:
        raise B2SError("silence_db %r gives an energy floor outside int64" % silence_db)
    return {"win": win, "hop": hop, "tau_min": tau_min, "tau_max": tau_max, "threshold": float(threshold), "min_energy": floor,
            "sr": sr}


def _wav_batch(wavs, lengths, device, dtype, what="wavs"):
    """Padded [B, Lmax] array or tensor, or a list of 1-D arrays (lengths=None: their own) -> (contiguous [B, Lmax] device tensor of
    `dtype`, lengths as Python ints)."""
    if isinstance(wavs, (list, tuple)):
        rows = [ragged.as_tensor(w).reshape(-1) for w in wavs]
        n = [int(r.numel()) for r in rows]
        t = torch.zeros(len(rows), max(n + [0]), dtype=dtype, device=device)
        for i, r in enumerate(rows):
            t[i, :n[i]] = r.to(device=device, dtype=dtype)
        if lengths is None:
            return t, n
        wavs = t
    t = ragged.as_tensor(wavs)
    if t.dim() != 2:
        raise B2SError("%s must be [B, Lmax], got %s" % (what, tuple(t.shape)))
    if lengths is None:
        raise B2SError("%s given as a padded array needs its lengths" % what)
    B, Lmax = int(t.shape[0]), int(t.shape[1])
    if isinstance(lengths, torch.Tensor):
        lengths = lengths.detach().cpu().numpy()
    n = [int(v) for v in np.asarray(lengths).reshape(-1)]
    if len(n) != B:
        raise B2SError("%d lengths for a batch of %d %s" % (len(n), B, what))
    if any(v < 0 or v > Lmax for v in n):
        raise B2SError("every length must be in 0..Lmax=%d samples (got %s)" % (Lmax, n))
    return t.to(device=device, dtype=dtype).contiguous(), n


def quantize_batch(wavs, lengths=None):
    """b2s_f0_quantize: fp32 waveforms [B, Lmax] (array, tensor on any device, or a list of 1-D arrays) with their sample counts ->
    dict of device tensors pcm [B, Lmax] int16 (zero past each length; the samples save_wav writes), peak [B] f32 and status [B]
    (FAILED: a NaN or Inf among the samples), and the host list `lengths`.  No host read."""
    lib = load()
    device = _device(wavs)
    wav, n = _wav_batch(wavs, lengths, device, torch.float32)
    B, Lmax = int(wav.shape[0]), int(wav.shape[1])
    pcm = torch.empty(B, Lmax, dtype=torch.int16, device=device)
    peak = torch.empty(B, dtype=torch.float32, device=device)
    status = torch.empty(B, dtype=torch.int32, device=device)
    if B:
        lens = torch.tensor(n, dtype=torch.int32).to(device)
        check(lib.b2s_f0_quantize(nptr(wav), nptr(lens), B, Lmax, nptr(pcm), nptr(peak), nptr(status), stream(device)))
    return {"pcm": pcm, "peak": peak, "status": status, "lengths": n}


def yin_batch(wavs_or_pcm, lengths=None, hp=None, return_cmnd=False, **params):
    """YIN on a batch: int16 PCM [B, Lmax] is taken as it is, anything else goes through quantize_batch first.  `params` are those
    of yin_params.  Returns a dict: device tensors f0 [total] f64 (0 = unvoiced), tau [total] int32, aper [total] f64 packed by
    frame_offsets (host array [B + 1], frame_offsets_device its copy), frames (host list, 1 + L // hop), status [B] device int32
    (the quantiser's FAILED handed on), pcm, lengths, params, and with return_cmnd cmnd [total, tau_max + 1] f64.  No host read."""
    lib = load()
    prm = yin_params(hp, **params)
    device = _device(wavs_or_pcm)
    is_pcm = (isinstance(wavs_or_pcm, torch.Tensor) and wavs_or_pcm.dtype == torch.int16) or \
        (isinstance(wavs_or_pcm, np.ndarray) and wavs_or_pcm.dtype == np.int16)
    qstatus = None
    if is_pcm:
        pcm, n = _wav_batch(wavs_or_pcm, lengths, device, torch.int16, "pcm")
    else:
        q = quantize_batch(wavs_or_pcm, lengths)
        pcm, n, qstatus = q["pcm"], q["lengths"], q["status"]
    B, Lmax = int(pcm.shape[0]), int(pcm.shape[1])
    frames = [1 + v // prm["hop"] for v in n]
    off_h, off = ragged.offsets(frames, device)
    total = int(off_h[-1])
    f0 = torch.empty(total, dtype=torch.float64, device=device)
    tau = torch.empty(total, dtype=torch.int32, device=device)
    aper = torch.empty(total, dtype=torch.float64, device=device)
    cm = torch.empty(total, prm["tau_max"] + 1, dtype=torch.float64, device=device) if return_cmnd else None
    status = torch.empty(B, dtype=torch.int32, device=device)
    if B:
        lens = torch.tensor(n, dtype=torch.int32).to(device)
        check(lib.b2s_f0_yin(nptr(pcm), nptr(lens), nptr(off), total, B, Lmax, prm["win"], prm["hop"], prm["tau_min"], prm["tau_max"],
                             prm["threshold"], prm["min_energy"], prm["sr"], nptr(f0), nptr(tau), nptr(aper), nptr(cm), nptr(status),
                             stream(device)))
        if qstatus is not None:
            status = torch.maximum(status, qstatus)
    out = {"f0": f0, "tau": tau, "aper": aper, "frame_offsets": off_h, "frame_offsets_device": off, "frames": frames,
           "status": status, "pcm": pcm, "lengths": n, "params": prm}
    if return_cmnd:
        out["cmnd"] = cm
    return out


def f0(wav, hp=None, **params):
    """F0 track of one utterance: NumPy waveform -> [1 + len // hop] float64 in Hz, 0 for unvoiced frames."""
    wav = np.asarray(wav, dtype=np.float32)
    if wav.ndim != 1:
        raise B2SError("wav must be 1-D, got %s" % (wav.shape,))
    out = yin_batch(wav[None], [wav.shape[0]], hp=hp, **params)
    if int(out["status"].cpu()[0]) == FAILED:
        raise B2SError("the waveform holds a NaN or Inf")
    return out["f0"].cpu().numpy()


def score_packed(x, y, kept_x, kx_offsets, kept_y, ky_offsets, path, path_offsets, path_len, dtw_status, gross_ratio=0.2):
    """b2s_f0_score on device data: x / y are yin_batch results (f0, tau, frame_offsets_device), kept_* int32 frame numbers packed by
    the B + 1 device offsets k*_offsets, path [total_path, 2] int32 with its B + 1 device offsets, path_len [B], dtw_status [B].
    No host read.  Returns device tensors scores [B, 5] f64, counts [B, 4] int32, status [B] int32."""
    lib = load()
    device = path_len.device
    B = int(path_len.numel())
    scores = torch.empty(B, 5, dtype=torch.float64, device=device)
    counts = torch.empty(B, 4, dtype=torch.int32, device=device)
    status = torch.empty(B, dtype=torch.int32, device=device)
    check(lib.b2s_f0_score(nptr(x["f0"]), nptr(x["tau"]), nptr(x["frame_offsets_device"]), int(x["f0"].numel()),
                           nptr(y["f0"]), nptr(y["tau"]), nptr(y["frame_offsets_device"]), int(y["f0"].numel()),
                           nptr(kept_x), nptr(kx_offsets), int(kept_x.numel()), nptr(kept_y), nptr(ky_offsets), int(kept_y.numel()),
                           B, nptr(path), nptr(path_offsets), int(path.shape[0]), nptr(path_len), nptr(dtw_status),
                           float(gross_ratio), nptr(scores), nptr(counts), nptr(status), stream(device)))
    return scores, counts, status


def kept_frames(mels, lengths, device=None, what="mels"):
    """The frames the MCD call keeps (row maximum > 0) of a padded mel batch: (int32 device tensor of frame numbers within their
    utterance, packed in order, and the per-utterance counts as an int64 device tensor [B])."""
    rows, off, _ = mcd.pack_batch(mels, lengths, device, what)
    B = int(off.numel()) - 1
    n = (off[1:] - off[:-1]).to(torch.int64)
    utt = torch.repeat_interleave(torch.arange(B, device=rows.device), n)
    idx = torch.nonzero(rows.max(dim=1).values > 0).reshape(-1)
    u = utt[idx]
    return (idx - off.to(torch.int64)[u]).to(torch.int32), torch.bincount(u, minlength=B)


def _vocode(mels, lengths, device, n_iter, hp):
    """mel2wav_batch on the utterances of at least 2 frames; the others get an empty waveform.  -> ([B, Lmax] f32, lengths)."""
    t = ragged.as_batch(mels, device, "mels")
    n = ragged.lengths(lengths, int(t.shape[0]), int(t.shape[1]), "lengths")
    hop = int(default_hp(hp).hop_length)
    wl = [hop * (v - 1) if v >= 2 else 0 for v in n]
    wav = torch.zeros(len(n), max(wl + [0]), dtype=torch.float32, device=device)
    sel = [b for b, v in enumerate(n) if v >= 2]
    if sel:
        w, _ = mel2wav_batch(t[sel].contiguous(), [n[b] for b in sel], n_iter=n_iter, hp=hp)
        wav[sel, :w.shape[1]] = w[:, :wav.shape[1]]
    return wav, wl


def f0_dtw_details(preds, pred_lengths, targets, target_lengths, pred_wavs=None, target_wavs=None, order=13, radius=1, n_iter=None,
                   hp=None, gross_ratio=0.2, **yin):
    """Everything one F0 scoring call produces.  preds / targets: padded mels as mcd_dtw_details takes them (x = prediction, y =
    target).  pred_wavs / target_wavs: the waveforms of a side, as a list of 1-D arrays or a (padded [B, Lmax], lengths) pair; a side
    without them is vocoded by mel2wav_batch at n_iter (default hp.n_iter), so that both sides meet the same Griffin-Lim artefacts.
    The DTW path over the kept frames comes from mcd.mcd_dtw_details.  Returns a dict: scores [B, 5] f64 (rmse_hz, rmse_cents, vde,
    gpe, ffe; also under those names), counts [B, 4] int32 (steps, vuv, both, gross), status [B] (OK / EMPTY / FAILED, nothing
    raised), x / y (the yin_batch results: pcm, f0, tau, aper, frame_offsets, ...), kept_x / kept_y with kept_offsets_x /
    kept_offsets_y, path, path_offsets (host), path_len, and `mcd`, the details of the MCD call.  An utterance of fewer than 2 frames
    on a vocoded side makes its pair EMPTY."""
    hp = default_hp(hp)
    device = _device(preds, targets)
    d = mcd.mcd_dtw_details(preds, pred_lengths, targets, target_lengths, order=order, radius=radius, hp=hp)
    B = int(d["status"].numel())
    short = np.zeros(B, bool)
    sides = []
    for mels, lengths, wavs in ((preds, pred_lengths, pred_wavs), (targets, target_lengths, target_wavs)):
        if wavs is None:
            wav, wl = _vocode(mels, lengths, device, n_iter, hp)
            short |= np.asarray(wl) == 0
        elif isinstance(wavs, tuple):
            wav, wl = _wav_batch(wavs[0], wavs[1], device, torch.float32)
        else:
            wav, wl = _wav_batch(list(wavs), None, device, torch.float32)
        if len(wl) != B:
            raise B2SError("%d waveforms for a batch of %d pairs" % (len(wl), B))
        sides.append(yin_batch(wav, wl, hp=hp, **yin))
    x, y = sides
    kx, cx = kept_frames(preds, pred_lengths, device, "preds")
    ky, cy = kept_frames(targets, target_lengths, device, "targets")
    host = torch.stack([cx, d["voiced_x"].to(torch.int64), cy, d["voiced_y"].to(torch.int64)]).cpu().numpy()
    mcd_failed = d["status"] == mcd.FAILED
    agree = (host[0] == host[1]) & (host[2] == host[3])
    if not np.all(agree | mcd_failed.cpu().numpy()):
        raise B2SError("kept frames of pairs %s differ from the MCD call's counts" % np.nonzero(~agree)[0].tolist())
    dstat = d["dtw_status"].clone()
    if short.any():
        dstat[torch.from_numpy(short).to(device)] = EMPTY
    scores, counts, status = score_packed(x, y, kx, d["offsets_x"], ky, d["offsets_y"], d["path"], d["path_offsets_device"],
                                          d["path_len"], dstat, gross_ratio)
    failed = mcd_failed | (x["status"] == FAILED) | (y["status"] == FAILED)
    status = torch.where(failed, torch.full_like(status, FAILED), status)
    scores = torch.where((status == OK).unsqueeze(1), scores, torch.full_like(scores, float("nan")))
    counts = torch.where((status == OK).unsqueeze(1), counts, torch.zeros_like(counts))
    out = {"scores": scores, "counts": counts, "status": status, "x": x, "y": y, "kept_x": kx, "kept_y": ky,
           "kept_offsets_x": d["offsets_x"], "kept_offsets_y": d["offsets_y"], "path": d["path"], "path_offsets": d["path_offsets"],
           "path_len": torch.where(status == OK, d["path_len"], torch.zeros_like(d["path_len"])), "mcd": d}
    for i, k in enumerate(SCORES):
        out[k] = scores[:, i]
    for i, k in enumerate(COUNTS):
        out[k] = counts[:, i]
    return out


_WHY_FAILED = "a non-finite sample, or sizes that do not fit together"


def f0_dtw_batch(preds, pred_lengths, targets, target_lengths, pred_wavs=None, target_wavs=None, order=13, radius=1, n_iter=None,
                 hp=None, gross_ratio=0.2, **yin):
    """The F0 scores of every pair as a dict of [B] device tensors: rmse_hz, rmse_cents, vde, gpe, ffe (f64, NaN where the pair is
    EMPTY or no step has both sides voiced), steps, vuv, both, gross (int32) and status.  Raises B2SError when a pair FAILED.  An
    empty batch gives empty tensors."""
    if len(preds) == 0:
        device = _device(preds, targets)
        out = {k: torch.empty(0, dtype=torch.float64, device=device) for k in SCORES}
        out.update({k: torch.empty(0, dtype=torch.int32, device=device) for k in COUNTS + ("status",)})
        return out
    d = f0_dtw_details(preds, pred_lengths, targets, target_lengths, pred_wavs, target_wavs, order=order, radius=radius,
                       n_iter=n_iter, hp=hp, gross_ratio=gross_ratio, **yin)
    raise_failed(d["status"], "F0 after DTW", why=_WHY_FAILED)
    return {k: d[k] for k in SCORES + COUNTS + ("status",)}


def _records(out):
    """Host dicts of Python numbers, one per pair; None for an EMPTY pair."""
    host = {k: out[k].cpu().numpy() for k in SCORES + COUNTS + ("status",)}
    res = []
    for b in range(len(host["status"])):
        if int(host["status"][b]) != OK:
            res.append(None)
            continue
        r = {k: float(host[k][b]) for k in SCORES}
        r.update({k: int(host[k][b]) for k in COUNTS})
        res.append(r)
    return res


def calculate_f0_dtw(preds, pred_lengths, targets, target_lengths, **kwargs):
    """The list shape of calculate_mse_dtw: per pair a dict of Python floats (the five scores) and ints (the four counts), None where
    the pair is EMPTY."""
    if len(preds) == 0:
        return []
    return _records(f0_dtw_batch(preds, pred_lengths, targets, target_lengths, **kwargs))


# ------------------------------------------------------------------------------------------------------- re-scoring a finished eval

def score_eval_dir(eval_dir, zipfilepath, eval_meta=None, order=13, radius=1, batch=64, n_iter=None, hp=None, **yin):
    """Score every `<name>.npy` of eval_dir against member `<name>.npy` of the mels.zip, `batch` pairs per GPU call, both sides
    vocoded.  Returns the summary dict: overall and per-language means of the five scores over the scored records (a NaN, no step
    with both sides voiced, is left out of that score's mean), the counts (scored, empty, without a target) and the records."""
    hp = default_hp(hp)
    lang = rescore.languages(eval_meta, hp)
    records = []

    def score(part, preds, pl, targets, tl):
        out = f0_dtw_details(preds, pl, targets, tl, order=order, radius=radius, n_iter=n_iter, hp=hp, **yin)
        raise_failed(out["status"], "F0 after DTW", why=_WHY_FAILED)
        for n, r in zip(part, _records(out)):
            rec = {"name": n, "language": lang.get(n), "scored": r is not None}
            rec.update(r if r is not None else dict.fromkeys(SCORES + COUNTS))
            records.append(rec)
    no_target = rescore.walk(eval_dir, zipfilepath, batch, score)
    head = {"metric": "f0_dtw", "radius": "exact" if radius is None else int(radius)}
    res = rescore.summary(head, records, [r for r in records if r["scored"]], no_target, SCORES)
    for r in records:                                          # JSON has no NaN
        for k in SCORES:
            if r[k] is not None and math.isnan(r[k]):
                r[k] = None
    return res


@rescore.cli
def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m b2s_hip.f0",
                                 description="Re-score a finished eval with the F0 error after DTW (YIN) on the GPU.")
    rescore.add_arguments(ap, "eval_dir", "--data-dir", "--zipfilepath", "--eval-meta", "--radius", "--batch")
    ap.add_argument("--n-iter", type=int, help="Griffin-Lim iterations of the vocoder (default: hp.n_iter)")
    ap.add_argument("--fmin", type=float, default=60.0, help="lowest F0 in Hz")
    ap.add_argument("--fmax", type=float, default=500.0, help="highest F0 in Hz")
    ap.add_argument("--threshold", type=float, default=0.1, help="YIN's absolute threshold")
    ap.add_argument("--silence-db", type=float, default=-40.0, help="frames below this level (dB re full scale) are unvoiced")
    rescore.add_arguments(ap, "--json")
    a = ap.parse_args(argv)
    zipfilepath, eval_meta = rescore.inputs(a)
    radius = rescore.radius(a.radius)
    rescore.batch(a.batch)
    if a.n_iter is not None and a.n_iter < 0:
        raise rescore.UsageError("--n-iter must be >= 0 (got %d)" % a.n_iter)
    from hyperparams import hparams as hp
    yin = {"fmin": a.fmin, "fmax": a.fmax, "threshold": a.threshold, "silence_db": a.silence_db}
    try:
        yin_params(hp, **yin)
    except B2SError as e:
        raise rescore.UsageError(str(e))
    rescore.found("EVAL_DIR", a.eval_dir, isdir=True)
    rescore.found("mels.zip", zipfilepath)
    res = score_eval_dir(a.eval_dir, zipfilepath, eval_meta, radius=radius, batch=a.batch, n_iter=a.n_iter, hp=hp, **yin)
    return rescore.finish(res, a.json, ("records", "without_target"))


if __name__ == "__main__":
    sys.exit(main())
