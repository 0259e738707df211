"""ctypes binding of libb2s_pros.so (C ABI in include/b2s_pros.h): batched prosody targets on the GPU.

A FastSpeech-2-style student needs three targets per input unit: duration, pitch and energy.  b2s_hip.durations extracts the first;
this module adds the other two (DESIGN.md section n).  Pitch: YIN's frame-local pick (b2s_hip.f0) leaves holes and single-frame
voicing flips, so the track here is a Viterbi search over YIN's CMND matrix with the states "unvoiced" and "lag k", a banded
transition cost and a small bias towards short lags that keeps the path off the sub-octave.  Energy: the exact sum of squares of
the int16 PCM per frame.  Both are averaged over the byte or code-point units of a duration vector, with a continuous (linearly
interpolated) F0 contour for the units without a voiced frame.  Every result is bit-reproducible and the same for an utterance
alone or inside a batch.  There is no CPU fallback.

    python -m b2s_hip.prosody CHECKPOINT --data-dir DATA_DIR --out OUT_DIR [--meta FILE] [--batch 32] [--units bytes|chars]
                              [--n-iter N] [--hparams "a=1,b=2"]

extracts teacher-forced durations (b2s_hip.durations) for every utterance of a metadata file (default DATA_DIR/metadata.eval.txt)
whose mel is a member of DATA_DIR/mels.zip, vocodes the target mel and writes OUT_DIR/<name>.npz (duration, pitch, pitch_voiced,
voiced_frames, energy: one value per byte or per code point), OUT_DIR/prosody.jsonl (one line per utterance) and OUT_DIR/stats.json
(count, mean, std, min, max of pitch, log_pitch, energy and energy_db over the units with frames, overall and per language; the
logarithms over the units whose value is above 0).  An utterance whose status is not OK or NOVOICE gets its line and no .npz.
"""
import ctypes as C
import json
import math
import os
import sys
import zipfile

import numpy as np
import torch

from . import durations as dur
from . import f0 as f0mod
from . import ragged, rescore
from .cbind import EMPTY, FAILED, OK  # noqa: F401 (the status words are part of this module's surface)
from .cbind import B2SError, Library, default_hp, dptr, nptr, stream
from .ragged import as_tensor, lengths_i32

SHORT, NOVOICE = 3, 4                      # after OK, EMPTY, FAILED: more frames asked for than there are; no voiced frame
STATUS_NAMES = ("OK", "EMPTY", "FAILED", "SHORT", "NOVOICE")
MAX_WIN, MAX_LAGS, MAX_W, MAX_S = 2048, 512, 64, 1024
UNIT_SUMS = ("frames", "voiced", "f0_voiced_sum", "f0_cont_sum", "energy_sum")
TARGETS = ("pitch", "pitch_voiced", "energy")
STATS = ("pitch", "log_pitch", "energy", "energy_db")

P = C.c_void_p
_I = C.c_int
_D = C.c_double
_PROTOS = {
    "b2s_pros_version": (C.c_int, []),
    "b2s_pros_last_error": (C.c_char_p, []),
    "b2s_pros_ws_bytes": (C.c_size_t, [_I, _I, _I]),
    "b2s_pros_energy": (C.c_int, [P, P, P, _I, _I, _I, _I, _I, P, P, P]),
    "b2s_pros_track": (C.c_int, [P, P, C.c_int64, P, _I, _I, _I, _I, _I, _D, _D, _D, _D, _D, _I, P, P, P, P, P, C.c_size_t, P]),
    "b2s_pros_units": (C.c_int, [P, P, P, P, _I, P, P, P, _I, _I, P, P, P, P, P, P, P, P, P, C.c_size_t, P]),
}
_LIB = Library("libb2s_pros.so", _PROTOS, "b2s_pros_last_error")
LIB_PATH, EXPORTS, load, check, workspace = _LIB.path, _LIB.exports, _LIB.load, _LIB.check, _LIB.workspace

_TRACK_KEYS = ("u", "v", "lam", "mu", "W", "floor")


def _device(*arrays):
    return ragged.device("the prosody extraction", *arrays)


def track_params(hp=None, **overrides):
    """The search's parameters as a dict, checked.  Defaults: u = 0.3 (a frame spent unvoiced), v = 0.1 (a change of voicing), lam =
    0.02 (per lag of a jump, inside the band), mu = 0.0005 (per lag, the bias that keeps the path off the sub-octave), W = 8 (half
    width of the band) and floor = f0.yin_params(hp)['min_energy'] (a frame below it cannot be voiced)."""
    unknown = sorted(set(overrides) - set(_TRACK_KEYS))
    if unknown:
        raise B2SError("unknown track parameter(s) %s (expected %s)" % (unknown, list(_TRACK_KEYS)))
    prm = {"u": 0.3, "v": 0.1, "lam": 0.02, "mu": 0.0005, "W": 8, "floor": None}
    prm.update({k: v for k, v in overrides.items() if v is not None})
    if prm["floor"] is None:
        prm["floor"] = f0mod.yin_params(hp)["min_energy"]
    for k in ("u", "v", "lam", "mu"):
        prm[k] = float(prm[k])
        if not math.isfinite(prm[k]):
            raise B2SError("%s must be finite (got %r)" % (k, prm[k]))
    prm["W"], prm["floor"] = int(prm["W"]), int(prm["floor"])
    if not 0 <= prm["W"] <= MAX_W:
        raise B2SError("W must be in 0..%d (got %d)" % (MAX_W, prm["W"]))
    if not -2 ** 63 <= prm["floor"] < 2 ** 63:
        raise B2SError("floor %r is outside int64" % prm["floor"])
    return prm


# ------------------------------------------------------------------------------------------------------------------------ energy

def energy_batch(wavs_or_pcm, lengths=None, hp=None, win=None, hop=None):
    """b2s_pros_energy: int16 PCM ([B, Lmax], or a list of 1-D int16 arrays) is taken as it is, anything else goes through
    f0.quantize_batch first.  win / hop default
    to hp.win_length / hp.hop_length.  Returns a dict: the device tensor energy [total] int64 packed by frame_offsets (host array [B +
    1], frame_offsets_device its copy; 1 + L // hop frames per utterance, YIN's count), frames (host list), status [B] device int32
    (the quantiser's FAILED handed on), pcm, lengths, win, hop.  No host read."""
    lib = load()
    hp = default_hp(hp) if None in (win, hop) else hp
    win = int(hp.win_length if win is None else win)
    hop = int(hp.hop_length if hop is None else hop)
    if not 1 <= win <= MAX_WIN:
        raise B2SError("win must be in 1..%d (got %d)" % (MAX_WIN, win))
    if hop < 1:
        raise B2SError("hop must be >= 1 (got %d)" % hop)
    device = _device(wavs_or_pcm)
    def int16(a):
        return (isinstance(a, torch.Tensor) and a.dtype == torch.int16) or (isinstance(a, np.ndarray) and a.dtype == np.int16)
    is_pcm = int16(wavs_or_pcm) or (isinstance(wavs_or_pcm, (list, tuple)) and len(wavs_or_pcm) > 0 and all(int16(a) for a in wavs_or_pcm))
    qstatus = None
    if is_pcm:
        pcm, n = f0mod._wav_batch(wavs_or_pcm, lengths, device, torch.int16, "pcm")
    else:
        q = f0mod.quantize_batch(wavs_or_pcm, lengths)
        pcm, n, qstatus = q["pcm"], q["lengths"], q["status"]
    B, Lmax = int(pcm.shape[0]), int(pcm.shape[1])
    frames = [1 + v // hop for v in n]
    off_h, off = ragged.offsets(frames, device)
    total = int(off_h[-1])
    energy = torch.empty(total, dtype=torch.int64, device=device)
    status = torch.empty(B, dtype=torch.int32, device=device)
    if B:
        lens = torch.tensor(n, dtype=torch.int32).to(device)
        with torch.cuda.device(device):
            check(lib.b2s_pros_energy(nptr(pcm), nptr(lens), nptr(off), total, B, Lmax, win, hop, nptr(energy), nptr(status),
                                      stream(device)))
        if qstatus is not None:
            status = torch.maximum(status, qstatus)
    return {"energy": energy, "frame_offsets": off_h, "frame_offsets_device": off, "frames": frames, "status": status, "pcm": pcm,
            "lengths": n, "win": win, "hop": hop}


# ------------------------------------------------------------------------------------------------------------------------- track

def track_batch(yin, energy=None, hp=None, **params):
    """b2s_pros_track on a f0.yin_batch(..., return_cmnd=True) result.  `energy`: an energy_batch result or its int64 tensor [total];
    None computes it from yin['pcm'] with YIN's win and hop.  `params` are those of track_params; floor defaults to the min_energy
    the YIN call used.  Returns a dict of device tensors tau [total] int32 (0 = unvoiced), f0 [total] f64, score [B] f64, status [B]
    int32 (YIN's FAILED handed on), with frame_offsets, frame_offsets_device, frames and params.  No host read."""
    lib = load()
    if "cmnd" not in yin:
        raise B2SError("track_batch needs the CMND matrix: call f0.yin_batch(..., return_cmnd=True)")
    yp = yin["params"]
    if params.get("floor") is None:
        params = dict(params, floor=yp["min_energy"])
    prm = track_params(hp, **params)
    cm = yin["cmnd"]
    device = cm.device
    if energy is None:
        energy = energy_batch(yin["pcm"], yin["lengths"], win=yp["win"], hop=yp["hop"])
    en = energy["energy"] if isinstance(energy, dict) else as_tensor(energy).to(device=device, dtype=torch.int64).contiguous()
    total, K = int(cm.shape[0]), int(cm.shape[1])
    if int(en.numel()) != total:
        raise B2SError("%d energies for %d frames" % (int(en.numel()), total))
    off = yin["frame_offsets_device"]
    B = int(off.numel()) - 1
    tau = torch.empty(total, dtype=torch.int32, device=device)
    f0 = torch.empty(total, dtype=torch.float64, device=device)
    score = torch.empty(B, dtype=torch.float64, device=device)
    status = torch.empty(B, dtype=torch.int32, device=device)
    if B:
        nbytes = lib.b2s_pros_ws_bytes(total, yp["tau_min"], yp["tau_max"])
        ws = workspace(nbytes, device)
        with torch.cuda.device(device):
            check(lib.b2s_pros_track(nptr(cm), nptr(en), prm["floor"], nptr(off), total, B, K, yp["tau_min"], yp["tau_max"], yp["sr"],
                                     prm["u"], prm["v"], prm["lam"], prm["mu"], prm["W"], nptr(tau), nptr(f0), nptr(score),
                                     nptr(status), dptr(ws), nbytes, stream(device)))
        status = torch.maximum(status, (yin["status"] == FAILED).to(torch.int32) * FAILED)
    return {"tau": tau, "f0": f0, "score": score, "status": status, "frame_offsets": yin["frame_offsets"],
            "frame_offsets_device": off, "frames": yin["frames"], "params": prm}


# ------------------------------------------------------------------------------------------------------------------------- units

def unit_prosody(track, energy, durations, input_lengths, groups=None):
    """b2s_pros_units: a track_batch result, an energy_batch result (or its tensor), durations [B, S] integers with input_lengths [B]
    and optionally groups [B, S] (durations.code_point_groups).  Returns device tensors: cont [total] f64 (the continuous contour),
    frames, voiced [B, S] int32, f0_voiced_sum, f0_cont_sum [B, S] f64, energy_sum [B, S] int64, units, status [B] int32 (OK / EMPTY /
    FAILED / SHORT / NOVOICE, nothing raised; a track that FAILED is handed on), and the per-unit means as fp64 [B, S]: pitch =
    f0_cont_sum / frames, pitch_voiced = f0_voiced_sum / voiced, energy = energy_sum / frames, each 0 where its denominator is 0."""
    lib = load()
    device = track["f0"].device
    en = energy["energy"] if isinstance(energy, dict) else as_tensor(energy).to(device=device, dtype=torch.int64).contiguous()
    d = as_tensor(durations).to(device=device, dtype=torch.int32).contiguous()
    if d.dim() != 2:
        raise B2SError("durations must be [B, S], got %s" % (tuple(d.shape),))
    B, S = int(d.shape[0]), int(d.shape[1])
    off = track["frame_offsets_device"]
    if int(off.numel()) - 1 != B:
        raise B2SError("durations of %d utterances for a track of %d" % (B, int(off.numel()) - 1))
    total = int(track["f0"].numel())
    if int(en.numel()) != total:
        raise B2SError("%d energies for %d frames" % (int(en.numel()), total))
    g = None
    if groups is not None:
        g = as_tensor(groups).to(device=device, dtype=torch.int32).contiguous()
        if g.shape != d.shape:
            raise B2SError("groups must have the shape of the durations %s (got %s)" % (tuple(d.shape), tuple(g.shape)))
    n_in = lengths_i32(input_lengths, B, device, "input_lengths")
    out = {"cont": torch.empty(total, dtype=torch.float64, device=device)}
    for k in UNIT_SUMS:
        dtype = torch.float64 if k.startswith("f0") else torch.int64 if k == "energy_sum" else torch.int32
        out[k] = torch.empty(B, S, dtype=dtype, device=device)
    out["units"] = torch.empty(B, dtype=torch.int32, device=device)
    out["status"] = torch.empty(B, dtype=torch.int32, device=device)
    if B:
        ws = torch.empty(max(total, 1), dtype=torch.int32, device=device)
        with torch.cuda.device(device):
            check(lib.b2s_pros_units(nptr(track["f0"]), nptr(track["tau"]), nptr(en), nptr(off), total, nptr(d), nptr(n_in), dptr(g),
                                     B, S, nptr(out["cont"]), nptr(out["frames"]), nptr(out["voiced"]), nptr(out["f0_voiced_sum"]),
                                     nptr(out["f0_cont_sum"]), nptr(out["energy_sum"]), nptr(out["units"]), nptr(out["status"]),
                                     dptr(ws), 4 * int(ws.numel()), stream(device)))
        out["status"] = torch.where(track["status"] == FAILED, torch.full_like(out["status"], FAILED), out["status"])
    fr, vo = out["frames"].to(torch.float64), out["voiced"].to(torch.float64)
    zero = torch.zeros_like(fr)
    out["pitch"] = torch.where(fr > 0, out["f0_cont_sum"] / fr.clamp(min=1.0), zero)
    out["pitch_voiced"] = torch.where(vo > 0, out["f0_voiced_sum"] / vo.clamp(min=1.0), zero)
    out["energy"] = torch.where(fr > 0, out["energy_sum"].to(torch.float64) / fr.clamp(min=1.0), zero)
    return out


def prosody_targets(mels, lengths, durations, input_lengths, groups=None, wavs=None, n_iter=None, hp=None, **params):
    """Pitch and energy per input unit.  mels [B, T, n_mels] with lengths: the utterances the durations belong to; wavs: their
    waveforms as a list of 1-D arrays or a (padded [B, Lmax], lengths) pair, None: vocoded by vocoder.mel2wav_batch at n_iter
    (default hp.n_iter), as the F0 score does.  `params`: those of f0.yin_params and of track_params.  Runs YIN with the CMND
    matrix, the energy, the track and the units.  Returns the unit_prosody dict plus `yin`, `energy_frames` and `track` (the three
    calls' results)."""
    hp = default_hp(hp)
    device = _device(mels)
    tp = {k: params.pop(k) for k in _TRACK_KEYS if k in params}
    if wavs is None:
        wav, wl = f0mod._vocode(mels, lengths, device, n_iter, hp)
    elif isinstance(wavs, tuple):
        wav, wl = f0mod._wav_batch(wavs[0], wavs[1], device, torch.float32)
    else:
        wav, wl = f0mod._wav_batch(list(wavs), None, device, torch.float32)
    B = int(as_tensor(durations).shape[0])
    if len(wl) != B:
        raise B2SError("%d waveforms for durations of %d utterances" % (len(wl), B))
    yin = f0mod.yin_batch(wav, wl, hp=hp, return_cmnd=True, **params)
    en = energy_batch(yin["pcm"], yin["lengths"], win=yin["params"]["win"], hop=yin["params"]["hop"])
    track = track_batch(yin, en, hp=hp, **tp)
    out = unit_prosody(track, en, durations, input_lengths, groups)
    out.update(yin=yin, energy_frames=en, track=track)
    return out


# -------------------------------------------------------------------------------------------------------------------- command line

def describe(values):
    """count, mean, std, min, max of a list of numbers in host fp64 (None for the last four without a value)."""
    v = np.asarray(values, dtype=np.float64)
    if v.size == 0:
        return {"count": 0, "mean": None, "std": None, "min": None, "max": None}
    return {"count": int(v.size), "mean": float(v.mean()), "std": float(v.std()), "min": float(v.min()), "max": float(v.max())}


def unit_stats(per_utterance, win):
    """per_utterance: (language, frames, pitch, energy) per written utterance, arrays per unit.  -> {"overall": {...}, "languages":
    {...}}: describe() of pitch, log_pitch, energy and energy_db = 10 log10(energy / (win 32767^2)) over the units with frames > 0
    (the two logarithms over those of them whose value is above 0)."""
    def gather(rows):
        acc = {k: [] for k in STATS}
        for _, fr, pitch, en in rows:
            keep = np.asarray(fr) > 0
            p, e = np.asarray(pitch, np.float64)[keep], np.asarray(en, np.float64)[keep]
            acc["pitch"].append(p)
            acc["log_pitch"].append(np.log(p[p > 0]))
            acc["energy"].append(e)
            acc["energy_db"].append(10.0 * np.log10(e[e > 0] / (float(win) * 32767.0 ** 2)))
        return {k: describe(np.concatenate(v) if v else []) for k, v in acc.items()}
    by_language = {}
    for row in per_utterance:
        by_language.setdefault(str(row[0]), []).append(row)
    return {"overall": gather(per_utterance), "languages": {k: gather(v) for k, v in sorted(by_language.items())}}


def extract(model, rows, mels, hp, spk_ids, lang_ids, out_dir, batch=32, units="bytes", n_iter=None, languages=None):
    """Teacher-forced durations and prosody targets of the metadata rows, `batch` utterances per forward, in file order.  Writes
    OUT/<name>.npz for every utterance whose status is OK or NOVOICE, OUT/prosody.jsonl for all of them and OUT/stats.json; returns
    the records."""
    from . import corpus
    from .batching import collate
    os.makedirs(out_dir, exist_ok=True)
    languages = languages or {}
    records, written = [], []
    with open(os.path.join(out_dir, "prosody.jsonl"), "w", encoding="utf-8") as log:
        for lo in range(0, len(rows), batch):
            data = collate([corpus.make_example(r, mels, hp, spk_ids, lang_ids) for r in rows[lo:lo + batch]], hp)
            res = dur.teacher_forced_durations(model, data)
            groups = dur.code_point_groups(data["inputs"], data["input_lengths"]) if units == "chars" else None
            tg = prosody_targets(data["mel_targets"], data["target_lengths"], res["durations"], data["input_lengths"], groups,
                                 n_iter=n_iter, hp=hp)
            host = {k: res[k].cpu().numpy() for k in ("status", "layer", "head", "focus", "mono_focus")}
            host.update({"p_" + k: tg[k].cpu().numpy() for k in ("status", "units", "frames", "voiced") + TARGETS})
            for i, name in enumerate(data["names"]):
                status = int(host["status"][i]) if int(host["status"][i]) != OK else int(host["p_status"][i])
                rec = {"name": name, "layer": int(host["layer"][i]), "head": int(host["head"][i]), "focus": float(host["focus"][i]),
                       "mono_focus": None if math.isnan(host["mono_focus"][i]) else float(host["mono_focus"][i]),
                       "status": STATUS_NAMES[status], "frames": int(data["target_lengths"][i]), "units": 0, "voiced_share": None}
                if status in (OK, NOVOICE):
                    nu = int(host["p_units"][i])
                    fr, vo = host["p_frames"][i, :nu].astype(np.int32), host["p_voiced"][i, :nu].astype(np.int32)
                    rec["units"] = nu
                    rec["voiced_share"] = float(vo.sum()) / max(int(fr.sum()), 1)
                    np.savez(os.path.join(out_dir, name + ".npz"), duration=fr, pitch=host["p_pitch"][i, :nu],
                             pitch_voiced=host["p_pitch_voiced"][i, :nu], voiced_frames=vo, energy=host["p_energy"][i, :nu])
                    written.append((languages.get(name), fr, host["p_pitch"][i, :nu], host["p_energy"][i, :nu]))
                log.write(json.dumps(rec, ensure_ascii=False) + "\n")
                records.append(rec)
    with open(os.path.join(out_dir, "stats.json"), "w", encoding="utf-8") as f:
        json.dump(dict(unit_stats(written, int(hp.win_length)), units=units, utterances=len(written)), f, ensure_ascii=False, indent=1)
    return records


@rescore.cli
def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m b2s_hip.prosody",
                                 description="Extract duration, pitch and energy targets per byte or per code point on the GPU.")
    ap.add_argument("checkpoint", help="a model.ckpt-<step> file of the reference's format")
    ap.add_argument("--data-dir", required=True, help="directory of mels.zip, the metadata and lang_id.json / spk_id.json")
    ap.add_argument("--out", required=True, metavar="OUT_DIR", help="where <name>.npz, prosody.jsonl and stats.json go")
    ap.add_argument("--meta", help="metadata file (default: DATA_DIR/metadata.eval.txt)")
    ap.add_argument("--batch", type=int, default=32, help="utterances per forward")
    ap.add_argument("--units", default="bytes", help="bytes (one target per input id) or chars (per UTF-8 code point)")
    ap.add_argument("--n-iter", type=int, help="Griffin-Lim iterations of the vocoder (default: hp.n_iter)")
    ap.add_argument("--hparams", default="", help="hyper-parameter overrides, 'name=value,...'")
    a = ap.parse_args(argv)
    rescore.batch(a.batch)
    if a.units not in ("bytes", "chars"):
        raise rescore.UsageError("--units must be 'bytes' or 'chars' (got %r)" % a.units)
    if a.n_iter is not None and a.n_iter < 0:
        raise rescore.UsageError("--n-iter must be >= 0 (got %d)" % a.n_iter)
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
        records = extract(model, rows, mels, hp, ids.get("spk_id.json"), ids.get("lang_id.json"), a.out, a.batch, a.units, a.n_iter,
                          rescore.languages(meta, hp))
    finally:
        mels.close()
    print(json.dumps({"utterances": len(records), "written": sum(r["status"] in ("OK", "NOVOICE") for r in records),
                      "units": a.units, "out": a.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
