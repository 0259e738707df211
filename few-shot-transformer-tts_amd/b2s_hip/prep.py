"""Corpus preparation on the GPU: a directory of wavs -> proc_wavs/ (16 kHz mono) -> mels/ -> mels.zip and its metadata.

The reference's corpora/process_corpus.py (trim_audios, recollect_meta, build_mels, merge_datasets) with paths as arguments instead of
its hard-coded ones, without librosa.  The body of trim_audios runs batched in libb2s_vocoder.so (b2s_voc_prep_trim, C ABI in
include/b2s_vocoder.h; kernels in csrc/vocoder/prep.hip), the mels come from vocoder.wav2mel_batch.  There is no CPU fallback: CPU
tensors are refused and a missing library is an error.

    python -m b2s_hip.prep --corpus DIR=lang [--corpus DIR=lang ...] --packed DIR [--resample hip]

By default a file that is not 16 kHz mono is refused.  resample="hip" (--resample hip) switches on the first line of the reference's
trim_audios, librosa.load(wav_file, sr=16000): np.mean over the channels and resampy's 'kaiser_best' interpolation, batched in
libb2s_vocoder.so (b2s_voc_resample; kernels in csrc/vocoder/resample.hip).  The resampled batch stays on the device and goes straight
into the trimming.  Parity is to a NumPy restatement of the published algorithm (tests/resample_ref.py); librosa and resampy themselves
are not needed anywhere.

What is not built: the per-dataset converters, statistics(), collect_samples() and the max95v plot; PCM24 and FLAC are not read.  One deliberate deviation: a file whose 95th-percentile amplitude (or peak) is zero is skipped as `silent`; the
reference divides by zero there and writes NaNs.  proc_wavs are written as float32 wavs; the reference writes float64 where it padded
with np.zeros and float32 elsewhere -- the sample values are the same.
"""
import argparse
import glob
import io
import json
import logging
import os
import random
import struct
import zipfile
from collections import defaultdict

import numpy as np
import torch

from . import vocoder
from .cbind import stream
from .lib import B2SError, ptr

log = logging.getLogger(__name__)

SR = 16000
LEAD, TAIL = 1600, 2400
STATUS_OK, STATUS_GAP, STATUS_LENGTH, STATUS_SILENT = 0, 1, 2, 3
STATUS_NAMES = ("ok", "gap", "length", "silent")
WS_TRIM, WS_QUANTILE = 0, 1
MAX_BATCH = 64
MAX_BATCH_SAMPLES = int(20.5 * SR)        # Lmax of a shared batch; a longer file gets a batch of its own


# ------------------------------------------------------------------------------------------------------------------- batched calls

def _device_batch(wavs, lengths):
    if isinstance(wavs, np.ndarray):
        wavs = torch.from_numpy(np.ascontiguousarray(wavs, dtype=np.float32)).cuda()
    if wavs.dim() != 2:
        raise B2SError("wavs must be [B, Lmax], got %s" % (tuple(wavs.shape),))
    if wavs.dtype != torch.float32:
        raise B2SError("wavs must be float32, got %s" % wavs.dtype)
    ptr(wavs)                                          # refuses CPU / non-contiguous tensors
    B, Lmax = int(wavs.shape[0]), int(wavs.shape[1])
    samples = [int(n) for n in lengths]
    if len(samples) != B:
        raise B2SError("%d lengths for a batch of %d" % (len(samples), B))
    if any(n < 2 or n > Lmax for n in samples):
        raise B2SError("every length must be in 2..Lmax=%d samples (got %s)" % (Lmax, samples))
    return wavs, B, Lmax, torch.tensor(samples, dtype=torch.int32).to(wavs.device)


def _trim_device(wavs, lengths, gap_threshold):
    """One b2s_voc_prep_trim call, nothing synchronised: (out [B, Lmax + 4000] cuda fp32, meta [4, B] cuda int32 holding out_lengths,
    status, n_removed and the bit patterns of v95)."""
    lib = vocoder.load()
    if isinstance(gap_threshold, bool) or not isinstance(gap_threshold, (int, np.integer)):
        raise B2SError("gap_threshold must be an integer number of samples, got %r" % (gap_threshold,))
    wavs, B, Lmax, lens = _device_batch(wavs, lengths)
    device = wavs.device
    ws = vocoder.workspace(lib.b2s_voc_prep_ws_bytes(B, Lmax, WS_TRIM), device)
    out = torch.empty(B, Lmax + LEAD + TAIL, dtype=torch.float32, device=device)
    meta = torch.empty(4, B, dtype=torch.int32, device=device)
    vocoder.check(lib.b2s_voc_prep_trim(ptr(wavs), ptr(lens), B, Lmax, int(gap_threshold), ptr(out), ptr(meta[0]), ptr(meta[1]),
                                        ptr(meta[2]), ptr(meta[3]), ptr(ws), ws.numel(), stream(device)))
    return out, meta


def trim_audios_batch(wavs, lengths, gap_threshold=12288):
    """The body of the reference's trim_audios for every utterance of a padded batch [B, Lmax] (cuda tensor or NumPy) with per-utterance
    sample counts `lengths` (host sequence, every L_b in 2..Lmax).  Returns (out [B, Lmax + 4000] cuda fp32, zero past each out_length;
    out_lengths, status, n_removed as int32 NumPy arrays; v95 as a float32 NumPy array).  status: 0 ok, 1 gap, 2 length, 3 silent; of an
    utterance that is not ok only status and n_removed mean anything.  Runs on torch.cuda.current_stream(); the one read-back of the four
    small arrays at the end is the only synchronisation."""
    out, meta = _trim_device(wavs, lengths, gap_threshold)
    m = meta.cpu().numpy()
    return out, m[0].copy(), m[1].copy(), m[2].copy(), m[3].copy().view(np.float32)


def _check_resample(resample):
    if resample not in (None, "hip"):
        raise ValueError("unknown resample %r (None or 'hip')" % (resample,))


def resample_lengths(n, orig_sr):
    """(n_valid, n_out) of n samples at orig_sr brought to 16 kHz: resampy interpolates int(n * ratio) samples and librosa's fix_length
    pads with zeros to int(ceil(n * ratio)), both in Python floats with ratio = float(16000) / orig_sr."""
    ratio = float(SR) / orig_sr
    return int(n * ratio), int(np.ceil(n * ratio))


def resample_tile(orig_sr):
    """(outputs per workgroup, input samples staged per workgroup) of the resampling kernel for orig_sr: the rule of
    csrc/vocoder/resample.hip (make_plan), restated for tests and benchmarks that want rows around those sizes."""
    ratio = float(SR) / orig_sr
    step = int(min(1.0, ratio) * 512)
    tile = 4096
    while True:
        span = (int(np.ceil(tile * (1.0 / ratio))) + 2 * (32769 // step) + 4 + 3) // 4 * 4
        if span <= 8064 or tile == 256:
            return tile, span
        tile //= 2


def _resample_device(wavs, lengths, orig_sr):
    """One b2s_voc_resample call, nothing synchronised: (out [B, Lmax_out] cuda fp32, n_out as a list)."""
    lib = vocoder.load()
    if isinstance(orig_sr, bool) or not isinstance(orig_sr, (int, np.integer)):
        raise B2SError("orig_sr must be an integer number of Hz, got %r" % (orig_sr,))
    if isinstance(wavs, np.ndarray):
        wavs = torch.from_numpy(np.ascontiguousarray(wavs, dtype=np.float32)).cuda()
    if wavs.dim() not in (2, 3):
        raise B2SError("wavs must be [B, Lmax] or [B, Lmax, C], got %s" % (tuple(wavs.shape),))
    if wavs.dtype != torch.float32:
        raise B2SError("wavs must be float32, got %s" % wavs.dtype)
    ptr(wavs)                                          # refuses CPU / non-contiguous tensors
    B, Lmax = int(wavs.shape[0]), int(wavs.shape[1])
    channels = int(wavs.shape[2]) if wavs.dim() == 3 else 1
    samples = [int(n) for n in lengths]
    if len(samples) != B:
        raise B2SError("%d lengths for a batch of %d" % (len(samples), B))
    if any(n < 1 or n > Lmax for n in samples):
        raise B2SError("every length must be in 1..Lmax=%d samples (got %s)" % (Lmax, samples))
    device = wavs.device
    ws = vocoder.workspace(lib.b2s_voc_resample_ws_bytes(B, Lmax, channels, int(orig_sr)), device)
    counts = np.array([resample_lengths(n, int(orig_sr)) for n in samples], dtype=np.int32).reshape(B, 2)
    Lmax_out = max(1, int(counts[:, 1].max()))
    meta = torch.from_numpy(np.ascontiguousarray(np.concatenate([np.array(samples, np.int32)[:, None], counts], axis=1).T)).to(device)
    out = torch.empty(B, Lmax_out, dtype=torch.float32, device=device)
    vocoder.check(lib.b2s_voc_resample(ptr(wavs), ptr(meta[0]), B, Lmax, channels, int(orig_sr), ptr(meta[1]), ptr(meta[2]), Lmax_out,
                                       ptr(out), ptr(ws), ws.numel(), stream(device)))
    return out, [int(n) for n in counts[:, 1]]


def resample_batch(wavs, lengths, orig_sr):
    """librosa.load(..., sr=16000)'s arithmetic for every utterance of a padded batch (cuda tensor or NumPy, float32): [B, Lmax] mono or
    [B, Lmax, C] interleaved with C in 1..8, per-utterance frame counts `lengths` (host sequence, every L_b in 1..Lmax; the padding may
    hold anything), all at orig_sr Hz.  Channels are averaged like np.mean, then resampled with resampy's 'kaiser_best' filter; at
    orig_sr == 16000 the result is the down-mix bit for bit.  Returns (out [B, Lmax_out] cuda fp32, zero from int(L_b * ratio) on,
    out_lengths = int(ceil(L_b * ratio)) as an int32 NumPy array).  Runs on torch.cuda.current_stream() without synchronising."""
    out, n_out = _resample_device(wavs, lengths, orig_sr)
    return out, np.array(n_out, dtype=np.int32)


def abs_quantile_batch(wavs, lengths, intervals, fraction=0.95):
    """np.sort(np.abs(np.concatenate([y[s:e] for s, e in intervals_b])))[min(int(N * fraction), N - 1)] for every utterance of a padded
    batch, bit for bit: float32 NumPy [B] (0.0 where the intervals cover no sample).  `intervals` is a list of B integer [n_b, 2] arrays
    of ascending, disjoint [start, end) sample ranges."""
    lib = vocoder.load()
    wavs, B, Lmax, lens = _device_batch(wavs, lengths)
    if len(intervals) != B:
        raise B2SError("%d interval lists for a batch of %d" % (len(intervals), B))
    ivs = [np.asarray(iv, dtype=np.int64).reshape(-1, 2) for iv in intervals]
    NI = max(1, max(len(iv) for iv in ivs))
    pad = np.zeros((B, NI, 2), np.int32)
    for b, iv in enumerate(ivs):
        pad[b, :len(iv)] = np.clip(iv, 0, Lmax)
    device = wavs.device
    iv_dev = torch.from_numpy(pad).to(device)
    n_dev = torch.tensor([len(iv) for iv in ivs], dtype=torch.int32).to(device)
    ws = vocoder.workspace(lib.b2s_voc_prep_ws_bytes(B, Lmax, WS_QUANTILE), device)
    out = torch.empty(B, dtype=torch.float32, device=device)
    vocoder.check(lib.b2s_voc_prep_abs_quantile(ptr(wavs), ptr(lens), B, Lmax, ptr(iv_dev), ptr(n_dev), NI, float(fraction), ptr(out),
                                                ptr(ws), ws.numel(), stream(device)))
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------------- WAV I/O

_PCM, _FLOAT, _EXTENSIBLE = 1, 3, 0xFFFE


def _riff_chunks(path):
    """(fmt fields, offset and size of the data chunk) of a RIFF/WAVE file."""
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:] != b"WAVE":
            raise B2SError("%s is not a RIFF/WAVE file" % path)
        fmt = data = None
        while True:
            ck = f.read(8)
            if len(ck) < 8:
                break
            tag, size = ck[:4], struct.unpack("<I", ck[4:])[0]
            if tag == b"fmt ":
                body = f.read(size)
                if len(body) < 16:
                    raise B2SError("%s: truncated fmt chunk" % path)
                code, channels, rate, _, align, bits = struct.unpack("<HHIIHH", body[:16])
                if code == _EXTENSIBLE and len(body) >= 26:
                    code = struct.unpack("<H", body[24:26])[0]
                fmt = {"format": code, "channels": channels, "rate": rate, "align": align, "bits": bits}
                f.seek(size & 1, 1)
            elif tag == b"data":
                data = (f.tell(), size)
                break
            else:
                f.seek(size + (size & 1), 1)
        if fmt is None or data is None:
            raise B2SError("%s: no fmt or no data chunk" % path)
        end = os.path.getsize(path)
        return fmt, data[0], min(data[1], end - data[0])


def wav_info(path):
    """(sample rate, channels, frames) from the header alone."""
    fmt, _, size = _riff_chunks(path)
    return fmt["rate"], fmt["channels"], size // max(1, fmt["align"])


def read_wav(path):
    """(samples, sample rate) of a PCM16, PCM32, float32 or float64 wav: float32 [frames] for mono, [frames, channels] otherwise;
    integer samples are divided by 2^15 / 2^31."""
    fmt, off, size = _riff_chunks(path)
    kinds = {(_PCM, 16): ("<i2", 32768.0), (_PCM, 32): ("<i4", 2147483648.0), (_FLOAT, 32): ("<f4", None), (_FLOAT, 64): ("<f8", None)}
    key = (fmt["format"], fmt["bits"])
    if key not in kinds:
        raise B2SError("%s: unsupported sample format (tag %d, %d bits); PCM16, PCM32, float32 and float64 are read" % ((path,) + key))
    dtype, div = kinds[key]
    width = fmt["bits"] // 8 * fmt["channels"]
    with open(path, "rb") as f:
        f.seek(off)
        raw = np.frombuffer(f.read(size - size % width), dtype=dtype)
    y = raw.astype(np.float32) if div is None else (raw.astype(np.float64) / div).astype(np.float32)
    if fmt["channels"] != 1:
        y = y.reshape(-1, fmt["channels"])
    return y, fmt["rate"]


def _refuse_unless_16k_mono(path, rate, channels):
    if rate != SR or channels != 1:
        raise B2SError("%s is %d Hz with %d channel(s); only %d Hz mono is accepted -- resampling and down-mixing are not built, "
                       "convert the file first" % (path, rate, channels, SR))


def load_wav(path, resample=None):
    """librosa.load(path, sr=16000) for a file that already is 16 kHz mono; any other file is refused, unless resample="hip": then the
    channels are averaged and the signal resampled to 16 kHz on the GPU (resample_batch)."""
    _check_resample(resample)
    rate, channels, _ = wav_info(path)
    if resample is None or (rate == SR and channels == 1):
        _refuse_unless_16k_mono(path, rate, channels)
        return read_wav(path)[0]
    y = read_wav(path)[0]
    if y.shape[0] == 0:
        return np.zeros(0, np.float32)
    out, n_out = resample_batch(y[None], [y.shape[0]], rate)
    return out[0, :n_out[0]].cpu().numpy()


def write_wav_float32(path, y, sr=SR):
    """Mono WAVE_FORMAT_IEEE_FLOAT file of float32 samples."""
    y = np.ascontiguousarray(np.asarray(y).reshape(-1), dtype="<f4")
    data = y.tobytes()
    fmt = struct.pack("<HHIIHH", _FLOAT, 1, int(sr), int(sr) * 4, 4, 32)
    fact = struct.pack("<I", y.shape[0])
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"fact" + struct.pack("<I", 4) + fact + b"data" + \
        struct.pack("<I", len(data)) + data
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
    return path


# ------------------------------------------------------------------------------------------------------------ corpus-level functions

def _corpus_name(corpus_dir):
    return os.path.basename(os.path.normpath(corpus_dir))


def default_gap_threshold(corpus_name):
    """The reference's rule: 16000 samples for pt_br and the caito* / css10* corpora, 12288 for every other."""
    if corpus_name == "pt_br" or corpus_name.startswith("caito") or corpus_name.startswith("css10"):
        return 16000
    return 12288


def default_min_speaker_samples(corpus_name):
    return 50 if corpus_name.startswith("google") else 100


def suffix_language(corpus_name):
    """The language of a google* / caito* corpus is spelled in the last five characters of its name, '_' standing for '-'
    (google_xx_yy -> xx-yy)."""
    return corpus_name[-5:].replace("_", "-")


def _length_sorted_batches(items):
    """items: (length, payload) pairs -> lists of payloads, ascending by length, at most MAX_BATCH per list and no list mixing a file
    above MAX_BATCH_SAMPLES with another."""
    items = sorted(items, key=lambda it: (it[0], it[1]))
    batches, cur = [], []
    for n, payload in items:
        if n > MAX_BATCH_SAMPLES:
            if cur:
                batches.append(cur)
                cur = []
            batches.append([payload])
            continue
        cur.append(payload)
        if len(cur) == MAX_BATCH:
            batches.append(cur)
            cur = []
    if cur:
        batches.append(cur)
    return batches


def _padded(ws):
    pad = np.zeros((len(ws), max(len(w) for w in ws)) + ws[0].shape[1:], np.float32)
    for i, w in enumerate(ws):
        pad[i, :len(w)] = w
    return pad


def _write_trimmed(batch, trimmed, out_dir, res):
    """The files of one trimmed batch (the result of trim_audios_batch for the paths in `batch`) and their counts."""
    out, out_lens, status, n_removed, v95 = trimmed
    out = out.cpu().numpy()
    for i, path in enumerate(batch):
        wav_name = os.path.basename(path)
        if n_removed[i] > 1:
            log.info("%s trimmed %d segments", wav_name, n_removed[i])
        if status[i] == STATUS_GAP:
            log.info("Skipped %s with gap", wav_name)
            res["n_gap"] += 1
        elif status[i] == STATUS_LENGTH:
            log.info("Skipped %s with length %.2f", wav_name, out_lens[i] / float(SR))
            res["n_len"] += 1
        elif status[i] == STATUS_SILENT:
            log.info("Skipped %s as silent", wav_name)
            res["n_silent"] += 1
        else:
            write_wav_float32(os.path.join(out_dir, wav_name), out[i, :out_lens[i]])
            res["max95v"].append(float(v95[i]))
            continue
        res["n_skip"] += 1


def trim_audios(corpus_dir, gap_threshold=None, resample=None):
    """wavs/*.wav of one corpus -> proc_wavs/*.wav (float32): noise spikes at either end removed, files with a long inner gap skipped,
    the 95th-percentile amplitude of the voiced part scaled to 0.244, 1600 / 2400 samples of margin, files outside 1..20 s skipped.
    gap_threshold=None applies the reference's rule by corpus name.  A corpus whose proc_wavs/ exists is left alone (returns None).
    A file that is not 16 kHz mono is refused, unless resample="hip": then such files are batched by (rate, channels) and by the length
    they will have at 16 kHz, down-mixed and resampled on the device (resample_batch) and trimmed from there.
    Returns {"n_files", "n_skip", "n_gap", "n_len", "n_silent", "max95v": [v95 of every file written]}."""
    _check_resample(resample)
    name = _corpus_name(corpus_dir)
    out_dir = os.path.join(corpus_dir, "proc_wavs")
    if os.path.exists(out_dir):
        log.info("%s: proc_wavs exists, skipped", name)
        return None
    thres = default_gap_threshold(name) if gap_threshold is None else gap_threshold
    files = sorted(glob.glob(os.path.join(corpus_dir, "wavs", "*.wav")))
    log.info("%s %d files", name, len(files))
    res = {"n_files": len(files), "n_skip": 0, "n_gap": 0, "n_len": 0, "n_silent": 0, "max95v": []}
    items, foreign = [], defaultdict(list)
    for path in files:
        rate, channels, frames = wav_info(path)
        if resample is None or (rate == SR and channels == 1):
            _refuse_unless_16k_mono(path, rate, channels)
        else:
            n_out = resample_lengths(frames, rate)[1]
            if n_out >= 2:
                foreign[(rate, channels)].append((n_out, path))
                continue
            frames = n_out
        if frames < 2:
            log.info("Skipped %s with length %.2f", os.path.basename(path), frames / float(SR))
            res["n_len"] += 1
            res["n_skip"] += 1
            continue
        items.append((frames, path))
    os.makedirs(out_dir)
    for batch in _length_sorted_batches(items):
        ws = [read_wav(p)[0] for p in batch]
        _write_trimmed(batch, trim_audios_batch(_padded(ws), [len(w) for w in ws], thres), out_dir, res)
    for (rate, channels), group in sorted(foreign.items()):
        for batch in _length_sorted_batches(group):              # the batch rule applies to the lengths at 16 kHz
            ws = [read_wav(p)[0] for p in batch]
            dev, n_out = _resample_device(_padded(ws), [len(w) for w in ws], rate)
            _write_trimmed(batch, trim_audios_batch(dev, n_out, thres), out_dir, res)
    log.info("Total skipped %d files (%d for gap, %d for length, %d silent)", res["n_skip"], res["n_gap"], res["n_len"], res["n_silent"])
    return res


def recollect_meta(corpus_dir, min_speaker_samples=None):
    """Rewrite metadata.csv (`name|text|speaker|lang`, name = `<speaker>_<id>`) to the utterances that have a proc_wavs file, are no
    duplicate (text, speaker) and whose speaker keeps at least min_speaker_samples of them (default: 50 for google*, else 100)."""
    name = _corpus_name(corpus_dir)
    meta = os.path.join(corpus_dir, "metadata.csv")
    with open(meta, encoding="utf-8") as f:
        lines = f.read().splitlines()
    kept, seen, per_spk = [], set(), defaultdict(int)
    n_miss = n_dup = 0
    for line in lines:
        cols = line.split("|")
        if len(cols[0].split("_")) != 2:
            raise B2SError("%s: utterance name %r is not <speaker>_<id>" % (meta, cols[0]))
        if (cols[1], cols[2]) in seen:
            n_dup += 1
            continue
        seen.add((cols[1], cols[2]))
        if os.path.exists(os.path.join(corpus_dir, "proc_wavs", cols[0] + ".wav")):
            per_spk[cols[0].split("_")[0]] += 1
            kept.append(cols)
        else:
            n_miss += 1
    thres = default_min_speaker_samples(name) if min_speaker_samples is None else min_speaker_samples
    drop = set(s for s, n in per_spk.items() if n < thres)
    out, n_skip, dur = [], 0, 0.0
    for cols in kept:
        if cols[0].split("_")[0] in drop:
            n_skip += 1
            continue
        rate, _, frames = wav_info(os.path.join(corpus_dir, "proc_wavs", cols[0] + ".wav"))
        dur += frames / float(rate)
        out.append("|".join(cols) + "\n")
    log.info("%s: total %d missing, %d skipped, %d dup, %d spk, %d spk skipped, %.2fh", name, n_miss, n_skip, n_dup,
             len(per_spk) - len(drop), len(drop), dur / 3600)
    with open(meta, "w", encoding="utf-8") as f:
        f.writelines(out)
    return {"n_kept": len(out), "n_missing": n_miss, "n_skipped": n_skip, "n_dup": n_dup, "n_speakers": len(per_spk) - len(drop),
            "n_speakers_skipped": len(drop), "hours": dur / 3600}


def build_mels(corpus_dir, hp=None):
    """mels/<name>.npy = get_spectrograms(proc_wavs/<name>.wav) (float32 [1 + len // hop, n_mels]) for every line of metadata.csv."""
    os.makedirs(os.path.join(corpus_dir, "mels"), exist_ok=True)
    with open(os.path.join(corpus_dir, "metadata.csv"), encoding="utf-8") as f:
        names = [line.split("|")[0] for line in f.read().splitlines()]
    items = []
    for n in names:
        path = os.path.join(corpus_dir, "proc_wavs", n + ".wav")
        items.append((wav_info(path)[2], n))
    for batch in _length_sorted_batches(items):
        ws = [load_wav(os.path.join(corpus_dir, "proc_wavs", n + ".wav")) for n in batch]
        mels, frames = vocoder.wav2mel_batch(_padded(ws), [len(w) for w in ws], hp=hp)
        mels = mels.cpu().numpy()
        for i, n in enumerate(batch):
            np.save(os.path.join(corpus_dir, "mels", n + ".npy"), mels[i, :frames[i]])
    return len(names)


def merge_datasets(corpus_dirs, languages, packed_dir, n_eval=100):
    """mels.zip (members `<name>.npy`), lang_id.json, spk_id.json (first-seen order) and metadata.train.txt / metadata.eval.txt
    (`name.npy|frames|text|lang`; per language random.seed(0), shuffle, the first n_eval lines to eval, both halves sorted by name) in
    packed_dir.  `languages`: the language of every corpus, as a sequence parallel to corpus_dirs or a dict keyed by corpus name."""
    os.makedirs(packed_dir, exist_ok=True)
    if not isinstance(languages, dict):
        languages = dict(zip([_corpus_name(c) for c in corpus_dirs], languages))
    lang_samples, lang_to_id, spk_to_id = defaultdict(list), {}, {}
    with zipfile.ZipFile(os.path.join(packed_dir, "mels.zip"), "w") as mel_zip:
        for corpus in corpus_dirs:
            name = _corpus_name(corpus)
            if name not in languages:
                raise B2SError("no language given for corpus %s" % name)
            lang = languages[name]
            with open(os.path.join(corpus, "metadata.csv"), encoding="utf-8") as f:
                lines = [line.split("|") for line in f.read().splitlines()]
            log.info("%s %s %d samples", name, lang, len(lines))
            if lang not in lang_to_id:
                lang_to_id[lang] = len(lang_to_id)
            for cols in lines:
                spk = cols[0].split("_")[0]
                if spk not in spk_to_id:
                    spk_to_id[spk] = len(spk_to_id)
                mel = np.load(os.path.join(corpus, "mels", cols[0] + ".npy"))
                with io.BytesIO() as b:
                    np.save(b, mel)
                    mel_zip.writestr(cols[0] + ".npy", b.getvalue())
                lang_samples[lang].append("|".join([cols[0] + ".npy", str(mel.shape[0]), cols[1], lang]))
    with open(os.path.join(packed_dir, "lang_id.json"), "w") as f:
        json.dump(lang_to_id, f, indent=1)
    with open(os.path.join(packed_dir, "spk_id.json"), "w") as f:
        json.dump(spk_to_id, f, indent=1)
    train_samples, eval_samples = [], []
    for lang, lines in lang_samples.items():
        random.seed(0)
        random.shuffle(lines)
        ev, tr = lines[:n_eval], lines[n_eval:]
        tr.sort(key=lambda x: x.split("|")[0])
        ev.sort(key=lambda x: x.split("|")[0])
        train_samples.extend(tr)
        eval_samples.extend(ev)
    with open(os.path.join(packed_dir, "metadata.train.txt"), "w", encoding="utf-8") as f:
        f.write("\n".join(train_samples))
    with open(os.path.join(packed_dir, "metadata.eval.txt"), "w", encoding="utf-8") as f:
        f.write("\n".join(eval_samples))
    return {"n_train": len(train_samples), "n_eval": len(eval_samples), "languages": lang_to_id, "speakers": spk_to_id}


def main(argv=None):
    ap = argparse.ArgumentParser(description="wavs/ + metadata.csv of every corpus -> proc_wavs/, mels/ and the packed mels.zip")
    ap.add_argument("--corpus", action="append", required=True, metavar="DIR=lang", help="a corpus directory and its language; repeatable")
    ap.add_argument("--packed", required=True, help="output directory of mels.zip, the id maps and the metadata split")
    ap.add_argument("--gap-threshold", type=int, default=None, help="samples; default: the reference's rule by corpus name")
    ap.add_argument("--min-speaker-samples", type=int, default=None)
    ap.add_argument("--n-eval", type=int, default=100)
    ap.add_argument("--resample", choices=["hip"], default=None,
                    help="hip: down-mix and resample files that are not 16 kHz mono on the GPU; default: refuse them")
    a = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    dirs, langs = [], []
    for spec in a.corpus:
        d, sep, lang = spec.rpartition("=")
        if not sep or not d or not lang:
            ap.error("--corpus wants DIR=lang, got %r" % spec)
        dirs.append(d)
        langs.append(lang)
    import hyperparams
    hyperparams.hparams.override_from_dict(hyperparams.DEFAULTS)
    for d in dirs:
        trim_audios(d, a.gap_threshold, a.resample)
        recollect_meta(d, a.min_speaker_samples)
        build_mels(d)
    print(json.dumps(merge_datasets(dirs, langs, a.packed, a.n_eval)))


if __name__ == "__main__":
    main()
