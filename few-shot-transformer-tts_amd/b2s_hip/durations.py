"""ctypes binding of libb2s_dur.so (C ABI in include/b2s_dur.h): batched monotonic alignment search and byte durations on the GPU.

The third objective score of a TTS evaluation next to MCD and F0: rhythm.  An encoder-decoder attention map [S, T] becomes one frame
count per input byte by the monotonic path of the largest summed weight (DESIGN.md section m): it starts at the first byte, ends at
the last, never steps back and never skips, so its counts are durations, which the per-frame argmax of alignment.select_alignments
are not.  The map of the synthesized utterance and the map of the teacher-forced forward on the ground-truth mel give two duration
vectors; their error per byte or per code point (RMSE in frames and ms, MAE, rate ratio, Pearson r) is derived from twelve exact
integers.  The same search extracts per-byte durations from a trained model, as FastSpeech does to train a non-autoregressive
student.  Every result is bit-reproducible and the same for an utterance alone or inside a batch.  There is no CPU fallback.

    python -m b2s_hip.durations CHECKPOINT --data-dir DATA_DIR --out OUT_DIR [--meta FILE] [--batch 32] [--units bytes|chars]
                                [--hparams "a=1,b=2"]

extracts teacher-forced durations for every utterance of a metadata file (default DATA_DIR/metadata.eval.txt) whose mel is a member
of DATA_DIR/mels.zip: OUT_DIR/<name>.npy (int32 per byte or per code point, summing to the utterance's frames) and
OUT_DIR/durations.jsonl (name, layer, head, focus, mono_focus, status, frames, units); an utterance whose status is not OK gets its
line and no .npy.
"""
import ctypes as C
import json
import math
import os
import sys
import zipfile

import numpy as np
import torch

from . import alignment, ragged, rescore
from .cbind import EMPTY, FAILED, OK  # noqa: F401 (the status words are part of this module's surface)
from .cbind import B2SError, Library, dptr, nptr, stream
from .ragged import as_tensor, lengths_i32

SHORT = 3                                  # after OK, EMPTY, FAILED: fewer decoder frames than input bytes
STATUS_NAMES = ("OK", "EMPTY", "FAILED", "SHORT")
MAX_S = 1024
COUNTS = ("n", "sum_x", "sum_y", "sum_abs", "sum_sq", "sum_xx", "sum_yy", "sum_xy", "max_x", "max_y", "zero_x", "zero_y")
SCORES = ("rmse_frames", "rmse_ms", "mae_frames", "rate_ratio", "pearson")

P = C.c_void_p
_I = C.c_int
_PROTOS = {
    "b2s_dur_version": (C.c_int, []),
    "b2s_dur_last_error": (C.c_char_p, []),
    "b2s_dur_ws_bytes": (C.c_size_t, [_I, _I, _I]),
    "b2s_dur_mas": (C.c_int, [P, P, P, _I, _I, _I, P, P, P, P, P, C.c_size_t, P]),
    "b2s_dur_score": (C.c_int, [P, P, P, P, _I, _I, P, P, P]),
}
_LIB = Library("libb2s_dur.so", _PROTOS, "b2s_dur_last_error")
LIB_PATH, EXPORTS, load, check, workspace = _LIB.path, _LIB.exports, _LIB.load, _LIB.check, _LIB.workspace


def _device(*arrays):
    return ragged.device("the duration search", *arrays)


# --------------------------------------------------------------------------------------------------------------------- the search

def mas_batch(maps, input_lengths, dec_lengths):
    """b2s_dur_mas: maps [B, S, T] fp32 (array or tensor on any device; the `maps` of alignment.select_alignments as they are) with
    the encoder and decoder lengths -> dict of device tensors, queued on the current stream without synchronising: `path` [B, T]
    int32 (-1 from the decoder length on), `durations` [B, S] int32 (0 from the encoder length on), `score` [B] f64, `status` [B]
    int32 (OK / EMPTY / FAILED / SHORT, nothing raised) and `mono_focus` = score / max(dec_len, 1), the monotonic counterpart of
    select_alignments' focus."""
    lib = load()
    device = _device(maps)
    t = as_tensor(maps)
    if t.dim() != 3:
        raise B2SError("maps must be [B, S, T], got %s" % (tuple(t.shape),))
    t = t.to(device=device, dtype=torch.float32).contiguous()
    B, S, T = (int(v) for v in t.shape)
    enc = lengths_i32(input_lengths, B, device, "input_lengths")
    dec = lengths_i32(dec_lengths, B, device, "dec_lengths")
    path = torch.empty(B, T, dtype=torch.int32, device=device)
    durations = torch.empty(B, S, dtype=torch.int32, device=device)
    score = torch.empty(B, dtype=torch.float64, device=device)
    status = torch.empty(B, dtype=torch.int32, device=device)
    if B:
        nbytes = lib.b2s_dur_ws_bytes(B, S, T)
        ws = workspace(nbytes, device)
        with torch.cuda.device(device):
            check(lib.b2s_dur_mas(nptr(t), nptr(enc), nptr(dec), B, S, T, nptr(path), nptr(durations), nptr(score), nptr(status),
                                  dptr(ws), nbytes, stream(device)))
    return {"path": path, "durations": durations, "score": score, "status": status,
            "mono_focus": score / dec.clamp(min=1).to(torch.float64)}


def byte_durations(encdec, input_lengths, dec_lengths):
    """Durations per input byte from encoder-decoder attention maps: either the per-layer list of [B, H, S, T] arrays (eval_batch's
    or the teacher-forced forward's alignments['encdec']) or the single [B, 1, S, T] array that eval_batch returns under
    hp.align == "hip" (as it is, or as its list of one).  alignment.select_alignments picks the head plot_attn would draw (the only
    one, in the second form) and mas_batch searches its map.  Returns the mas_batch dict plus `layer`, `head` [B] int32 (-1: no head
    scores above 0; the search then runs on a map of zeros) and `focus` [B] f64."""
    layers = [encdec] if isinstance(encdec, (torch.Tensor, np.ndarray)) else list(encdec)
    sel = alignment.select_alignments(layers, input_lengths, dec_lengths)
    out = mas_batch(sel["maps"], input_lengths, dec_lengths)
    out.update(layer=sel["layer"], head=sel["head"], focus=sel["focus"])
    return out


def code_point_groups(inputs, input_lengths):
    """Unit ids for the duration error per character: inputs [B, S] byte ids of utils/text.py (array or tensor; the result stays on
    the tensor's device).  A UTF-8 continuation byte (0x80..0xBF) joins the unit of the byte before it; every other id, sos and eos
    included, starts a unit.  -> [B, S] int32, non-decreasing from 0 over each utterance's length and -1 past it."""
    ids = as_tensor(inputs)
    if ids.dim() != 2:
        raise B2SError("inputs must be [B, S], got %s" % (tuple(ids.shape),))
    B, S = int(ids.shape[0]), int(ids.shape[1])
    n = as_tensor(input_lengths).reshape(-1).to(device=ids.device, dtype=torch.int64)
    if n.numel() != B:
        raise B2SError("%d input_lengths for a batch of %d" % (n.numel(), B))
    starts = ~((ids >= 0x80) & (ids <= 0xBF))
    if S:
        starts[:, 0] = True
    groups = torch.cumsum(starts.to(torch.int32), dim=1, dtype=torch.int32) - 1
    past = torch.arange(S, device=ids.device).unsqueeze(0) >= n.unsqueeze(1)
    return groups.masked_fill(past, -1)


# ---------------------------------------------------------------------------------------------------------------------- the error

def scores_from_counts(counts, frame_ms):
    """The duration scores from the twelve integers of b2s_dur_score: counts [B, 12] (or [12]) NumPy int64 -> dict of float64 arrays
    [B]: rmse_frames = sqrt(sum_sq / n), rmse_ms = rmse_frames * frame_ms, mae_frames = sum_abs / n, rate_ratio = sum_x / sum_y (NaN
    for sum_y == 0) and pearson = (n sxy - sx sy) / sqrt((n sxx - sx^2) (n syy - sy^2)), whose numerator and factors are exact
    integers (NaN when a factor is 0: a side with the same duration everywhere).  A row with n == 0 is NaN throughout."""
    c = np.asarray(counts)
    if c.dtype != np.int64 or c.shape[-1] != len(COUNTS):
        raise B2SError("counts must be int64 [B, %d], got %s %s" % (len(COUNTS), c.dtype, c.shape))
    rows = c.reshape(-1, len(COUNTS))
    out = {k: np.full(len(rows), np.nan) for k in SCORES}
    for i, row in enumerate(rows):
        n, sx, sy, sabs, ssq, sxx, syy, sxy = (int(v) for v in row[:8])
        if n <= 0:
            continue
        out["rmse_frames"][i] = math.sqrt(ssq / n)
        out["rmse_ms"][i] = out["rmse_frames"][i] * float(frame_ms)
        out["mae_frames"][i] = sabs / n
        if sy:
            out["rate_ratio"][i] = sx / sy
        fx, fy = n * sxx - sx * sx, n * syy - sy * sy
        if fx > 0 and fy > 0:
            out["pearson"][i] = (n * sxy - sx * sy) / math.sqrt(fx * fy)
    return out if c.ndim == 2 else {k: v[0] for k, v in out.items()}


def duration_error_batch(dur_x, dur_y, input_lengths, groups=None, frame_ms=None):
    """b2s_dur_score: the duration error of x (prediction) against y (target), both [B, S] integers (arrays or tensors), per position
    or, with `groups` [B, S] (code_point_groups), per unit.  frame_ms defaults to hp.frame_shift_ms.  Returns `counts` [B, 12] int64
    and `status` [B] int32 (device tensors; EMPTY / FAILED rows hold zeros, nothing is raised) and, from the integers through
    scores_from_counts, the float64 NumPy arrays rmse_frames, rmse_ms, mae_frames, rate_ratio and pearson (NaN where the status is
    not OK).  The scores are read on the host, so this call waits for the stream."""
    lib = load()
    device = _device(dur_x, dur_y)
    if frame_ms is None:
        from hyperparams import hparams as hp
        frame_ms = hp.frame_shift_ms
    x, y = (as_tensor(d).to(device=device, dtype=torch.int32).contiguous() for d in (dur_x, dur_y))
    if x.dim() != 2 or x.shape != y.shape:
        raise B2SError("dur_x and dur_y must be [B, S] of one shape (got %s and %s)" % (tuple(x.shape), tuple(y.shape)))
    B, S = int(x.shape[0]), int(x.shape[1])
    g = None
    if groups is not None:
        g = as_tensor(groups).to(device=device, dtype=torch.int32).contiguous()
        if g.shape != x.shape:
            raise B2SError("groups must have the shape of the durations %s (got %s)" % (tuple(x.shape), tuple(g.shape)))
    enc = lengths_i32(input_lengths, B, device, "input_lengths")
    counts = torch.zeros(B, len(COUNTS), dtype=torch.int64, device=device)
    status = torch.empty(B, dtype=torch.int32, device=device)
    if B:
        with torch.cuda.device(device):
            check(lib.b2s_dur_score(nptr(x), nptr(y), nptr(enc), dptr(g), B, S, nptr(counts), nptr(status), stream(device)))
    out = {"counts": counts, "status": status}
    out.update(scores_from_counts(counts.cpu().numpy(), frame_ms))
    return out


# ---------------------------------------------------------------------------------------------------------- durations of a model

def _model_device(model):
    for p in model.parameters():
        return p.device
    raise B2SError("the model has no parameters")


def teacher_forced_durations(model, batch):
    """Durations the model assigns to the ground truth: the teacher-forced forward on batch['mel_targets'] (the dataloader's batch
    dict, NumPy arrays or tensors) under torch.no_grad() with the whole model in eval(), then byte_durations on its encoder-decoder
    alignments with input_lengths and target_lengths.  The model's training flag is put back.  Returns the byte_durations dict."""
    device = _model_device(model)
    if device.type != "cuda":
        raise B2SError("the duration search runs on the GPU only; the model is on %s" % device)
    keys = ("inputs", "input_lengths", "mel_targets", "target_lengths", "input_spk_ids", "input_language_vecs")
    args = {k: (None if batch.get(k) is None else as_tensor(batch[k]).to(device)) for k in keys}
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            out = model(**args)
            return byte_durations(out["alignments"]["encdec"], args["input_lengths"], args["target_lengths"])
    finally:
        model.train(was_training)


def eval_durations(model, batch, results):
    """Duration error of a synthesized batch against its ground truth.  `batch` is the dict eval_batch was given (with mel_targets
    and target_lengths), `results` what it returned (device_results=True or NumPy arrays; per-layer alignments or the selected map
    of hp.align == "hip").  The synthesized side's durations come from results['alignments'], the target side's from
    teacher_forced_durations; each side uses its own best head.  Returns a dict: `generated` and `target` (the byte_durations dicts,
    layer / head / focus of either choice included), `groups` (code_point_groups), `bytes` and `chars` (duration_error_batch per byte
    and per code point, x = generated, y = target) and `status` [B] int32 on the device: the first status that is not OK among the
    generated side's, the target side's and the error's.  Where it is not OK the scores of `bytes` and `chars` are NaN."""
    device = _model_device(model)
    n_in = as_tensor(results["input_lengths"] if results.get("input_lengths") is not None else batch["input_lengths"])
    gen = byte_durations(results["alignments"]["encdec"], n_in, results["generated_lengths"])
    selected = results["alignments"].get("selected") if isinstance(results["alignments"], dict) else None
    if selected is not None:                                  # the map was chosen inside eval_batch: that choice is the one to report
        for k in ("layer", "head", "focus"):
            gen[k] = as_tensor(selected[k]).to(device)
    tgt = teacher_forced_durations(model, batch)
    if gen["durations"].shape != tgt["durations"].shape:
        raise B2SError("the synthesized side has durations %s, the target side %s" % (tuple(gen["durations"].shape),
                                                                                     tuple(tgt["durations"].shape)))
    groups = code_point_groups(as_tensor(batch["inputs"]).to(device), n_in)
    out = {"generated": gen, "target": tgt, "groups": groups}
    status = torch.where(gen["status"] != OK, gen["status"], tgt["status"])
    for name, g in (("bytes", None), ("chars", groups)):
        err = duration_error_batch(gen["durations"], tgt["durations"], n_in, groups=g)
        status = torch.where(status != OK, status, err["status"])
        out[name] = err
    bad = (status != OK).cpu().numpy()
    for name in ("bytes", "chars"):
        for k in SCORES:
            out[name][k][bad] = np.nan
    out["status"] = status
    return out


# -------------------------------------------------------------------------------------------------------------------- command line

def unit_sums(durations, groups):
    """Host side of --units chars: the durations [n] summed over the units of groups [n] (non-decreasing from 0) -> int32."""
    return np.bincount(np.asarray(groups, np.int64), weights=np.asarray(durations, np.float64)).astype(np.int32)


def extract(model, rows, mels, hp, spk_ids, lang_ids, out_dir, batch=32, units="bytes"):
    """Teacher-forced durations of the metadata rows, `batch` utterances per forward, in file order.  Writes OUT/<name>.npy for every
    utterance whose status is OK and OUT/durations.jsonl for all of them; returns the records."""
    from . import corpus
    from .batching import collate
    os.makedirs(out_dir, exist_ok=True)
    records = []
    with open(os.path.join(out_dir, "durations.jsonl"), "w", encoding="utf-8") as log:
        for lo in range(0, len(rows), batch):
            data = collate([corpus.make_example(r, mels, hp, spk_ids, lang_ids) for r in rows[lo:lo + batch]], hp)
            res = teacher_forced_durations(model, data)
            host = {k: res[k].cpu().numpy() for k in ("durations", "status", "layer", "head", "focus", "mono_focus")}
            groups = code_point_groups(data["inputs"], data["input_lengths"]).numpy() if units == "chars" else None
            for i, name in enumerate(data["names"]):
                n, status = int(data["input_lengths"][i]), int(host["status"][i])
                rec = {"name": name, "layer": int(host["layer"][i]), "head": int(host["head"][i]), "focus": float(host["focus"][i]),
                       "mono_focus": None if math.isnan(host["mono_focus"][i]) else float(host["mono_focus"][i]),
                       "status": STATUS_NAMES[status], "frames": int(data["target_lengths"][i]), "units": 0}
                if status == OK:
                    d = host["durations"][i, :n].astype(np.int32)
                    if groups is not None:
                        d = unit_sums(d, groups[i, :n])
                    rec["units"] = int(len(d))
                    np.save(os.path.join(out_dir, name + ".npy"), d)
                log.write(json.dumps(rec, ensure_ascii=False) + "\n")
                records.append(rec)
    return records


@rescore.cli
def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m b2s_hip.durations",
                                 description="Extract teacher-forced durations per byte or per code point on the GPU.")
    ap.add_argument("checkpoint", help="a model.ckpt-<step> file of the reference's format")
    ap.add_argument("--data-dir", required=True, help="directory of mels.zip, the metadata and lang_id.json / spk_id.json")
    ap.add_argument("--out", required=True, metavar="OUT_DIR", help="where <name>.npy and durations.jsonl go")
    ap.add_argument("--meta", help="metadata file (default: DATA_DIR/metadata.eval.txt)")
    ap.add_argument("--batch", type=int, default=32, help="utterances per forward")
    ap.add_argument("--units", default="bytes", help="bytes (one duration per input id) or chars (per UTF-8 code point)")
    ap.add_argument("--hparams", default="", help="hyper-parameter overrides, 'name=value,...'")
    a = ap.parse_args(argv)
    rescore.batch(a.batch)
    if a.units not in ("bytes", "chars"):
        raise rescore.UsageError("--units must be 'bytes' or 'chars' (got %r)" % a.units)
    zipfilepath = os.path.join(a.data_dir, "mels.zip")
    meta = a.meta or os.path.join(a.data_dir, "metadata.eval.txt")
    for what, path in (("checkpoint", a.checkpoint), ("mels.zip", zipfilepath), ("metadata", meta)):
        rescore.found(what, path)
    from hyperparams import hparams as hp
    if a.hparams:
        hp.parse(a.hparams)
    ids = {}
    for name in ("spk_id.json", "lang_id.json"):
        path = os.path.join(a.data_dir, name)
        if os.path.isfile(path):
            with open(path, encoding="utf-8") as f:
                ids[name] = json.load(f)
        elif hp.multi_speaker or hp.multi_lingual:
            rescore.found(name, path)
    from transformer.tacotron import Tacotron
    from utils.checkpoint import load_model
    from . import corpus
    device = _device()
    model = Tacotron(hp)
    load_model(a.checkpoint, model, map_location="cpu")
    model = model.to(device)
    with zipfile.ZipFile(zipfilepath) as z:
        members = set(z.namelist())
    rows = [r for r in corpus.read_metadata(meta, hp.data_format) if r["n"] in members]      # listed without a mel: left out
    mels = corpus.MelZip(zipfilepath)
    try:
        records = extract(model, rows, mels, hp, ids.get("spk_id.json"), ids.get("lang_id.json"), a.out, a.batch, a.units)
    finally:
        mels.close()
    print(json.dumps({"utterances": len(records), "written": sum(r["status"] == "OK" for r in records), "units": a.units,
                      "out": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
