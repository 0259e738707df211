"""ctypes binding of libb2s_vocoder.so (C ABI in include/b2s_vocoder.h): batched Griffin-Lim vocoder, mel front end, silence
splitting / trimming, corpus preparation and resampling to 16 kHz on the GPU.

The reference's utils/audio.py surface (mel2wav, get_spectrograms, save_wav, trim_silence_intervals) and librosa.effects.split / trim
with librosa 0.6.0 semantics, run as HIP kernels for gfx950.  There is no CPU fallback: CPU tensors are refused and a missing library
is an error.  The vocoder and the mel front end have only n_fft 2048, win_length 800, hop_length 200 and 80 mels compiled in; other
values are refused by the library with a message naming the supported set.  The silence kernels take any frame_length in 2..8192 and
1 <= hop_length <= frame_length.
"""
import ctypes as C
import wave

import numpy as np
import torch

from . import ragged
from .cbind import Library, default_hp, stream
from .lib import B2SError, ptr

WS_MEL2WAV, WS_WAV2MEL = 0, 1


class Params(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("sr", "n_fft", "hop", "win", "n_mels")] + \
               [(n, C.c_float) for n in ("preemphasis", "ref_db", "max_db", "max_abs_value", "power")] + \
               [("symmetric_mel", C.c_int32)]


P = C.c_void_p
_PROTOS = {
    "b2s_voc_version": (C.c_int, []),
    "b2s_voc_last_error": (C.c_char_p, []),
    "b2s_voc_ws_bytes": (C.c_size_t, [C.POINTER(Params), C.c_int, C.c_int, C.c_int, C.c_int]),
    "b2s_voc_mel2wav": (C.c_int, [C.POINTER(Params), P, P, C.c_int, C.c_int, C.c_int, C.c_int, P, P, P, C.c_size_t, P]),
    "b2s_voc_wav2mel": (C.c_int, [C.POINTER(Params), P, P, P, C.c_int, C.c_int, C.c_int, P, P, P, C.c_size_t, P]),
    "b2s_voc_silence_ws_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "b2s_voc_silence_split": (C.c_int, [P, P, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, P, P, P, P, P, P, P, C.c_size_t, P]),
    "b2s_voc_silence_gather": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, P, P, P, P, P, P]),
    # corpus preparation (b2s_hip/prep.py)
    "b2s_voc_prep_ws_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "b2s_voc_prep_trim": (C.c_int, [P, P, C.c_int, C.c_int, C.c_int, P, P, P, P, P, P, C.c_size_t, P]),
    "b2s_voc_prep_abs_quantile": (C.c_int, [P, P, C.c_int, C.c_int, P, P, C.c_int, C.c_double, P, P, C.c_size_t, P]),
    # down-mix and resampling to 16 kHz (b2s_hip/prep.py)
    "b2s_voc_resample_ws_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "b2s_voc_resample": (C.c_int, [P, P, C.c_int, C.c_int, C.c_int, C.c_int, P, P, C.c_int, P, P, C.c_size_t, P]),
}
_LIB = Library("libb2s_vocoder.so", _PROTOS, "b2s_voc_last_error")
LIB_PATH, EXPORTS, load, check, workspace = _LIB.path, _LIB.exports, _LIB.load, _LIB.check, _LIB.workspace


def params(hp=None):
    hp = default_hp(hp)
    return Params(sr=int(hp.sr), n_fft=int(hp.n_fft), hop=int(hp.hop_length), win=int(hp.win_length), n_mels=int(hp.num_mels),
                  preemphasis=float(hp.preemphasis), ref_db=float(hp.ref_db), max_db=float(hp.max_db),
                  max_abs_value=float(hp.max_abs_value), power=float(hp.power), symmetric_mel=int(bool(hp.symmetric_mel)))


# ---------------------------------------------------------------------------------------------------------------- mel basis (host)

def _hz_to_mel(f):
    f = np.asanyarray(f, dtype=np.float64)
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_hz / f_sp + np.log(np.maximum(f, min_log_hz) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asanyarray(m, dtype=np.float64)
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, np.log(6.4) / 27.0
    min_log_mel = min_log_hz / f_sp
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


_basis_cache = {}


def mel_basis(hp=None):
    """librosa.filters.mel(sr, n_fft, n_mels) (Slaney scale, htk=False, norm=1): [n_mels, 1 + n_fft // 2] float64, cached."""
    hp = default_hp(hp)
    key = ("basis", int(hp.sr), int(hp.n_fft), int(hp.num_mels))
    if key not in _basis_cache:
        sr, n_fft, n_mels = key[1:]
        fftfreqs = np.linspace(0, sr / 2.0, 1 + n_fft // 2)
        mel_f = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(sr / 2.0), n_mels + 2))
        fdiff = np.diff(mel_f)
        ramps = mel_f[:, None] - fftfreqs[None, :]
        w = np.maximum(0.0, np.minimum(-ramps[:-2] / fdiff[:-1, None], ramps[2:] / fdiff[1:, None]))
        w *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
        w.flags.writeable = False
        _basis_cache[key] = w
    return _basis_cache[key]


def inverse_mel_basis(hp=None):
    """np.linalg.pinv(mel_basis): [1 + n_fft // 2, n_mels] float64, cached (the reference's mel_to_linear)."""
    hp = default_hp(hp)
    key = ("pinv", int(hp.sr), int(hp.n_fft), int(hp.num_mels))
    if key not in _basis_cache:
        inv = np.linalg.pinv(mel_basis(hp))
        inv.flags.writeable = False
        _basis_cache[key] = inv
    return _basis_cache[key]


def _device_tables(hp, device):
    """(basis [n_mels, n_bins], pinv^T [n_mels, n_bins]) as fp32 on `device`, uploaded once per device."""
    key = ("dev", int(hp.sr), int(hp.n_fft), int(hp.num_mels), str(device))
    if key not in _basis_cache:
        basis = torch.from_numpy(np.ascontiguousarray(mel_basis(hp), dtype=np.float32)).to(device)
        inv_t = torch.from_numpy(np.ascontiguousarray(inverse_mel_basis(hp).T, dtype=np.float32)).to(device)
        _basis_cache[key] = (basis, inv_t)
    return _basis_cache[key]


# ------------------------------------------------------------------------------------------------------------------- batched calls

def mel2wav_batch(mels, lengths, n_iter=None, hp=None):
    """Vocode a padded batch of normalised mels [B, Tmax, n_mels] (cuda tensor or NumPy) with per-utterance frame counts `lengths`
    (host sequence, every T_b >= 2).  Returns (wav [B, hop * (Tmax - 1)] cuda fp32, zero past each hop * (T_b - 1), wav_lengths).
    Runs on torch.cuda.current_stream() without synchronising; the workspace comes from the torch allocator."""
    hp = default_hp(hp)
    lib = load()
    n_iter = int(hp.n_iter if n_iter is None else n_iter)
    if isinstance(mels, np.ndarray):
        mels = torch.from_numpy(np.ascontiguousarray(mels, dtype=np.float32)).cuda()
    if mels.dim() != 3:
        raise B2SError("mels must be [B, Tmax, n_mels], got %s" % (tuple(mels.shape),))
    if mels.dtype != torch.float32:
        raise B2SError("mels must be float32, got %s" % mels.dtype)
    ptr(mels)                                          # refuses CPU / non-contiguous tensors before anything is uploaded
    B, Tmax = int(mels.shape[0]), int(mels.shape[1])
    frames = [int(t) for t in lengths]
    if len(frames) != B:
        raise B2SError("%d lengths for a batch of %d" % (len(frames), B))
    if any(t < 2 or t > Tmax for t in frames):
        raise B2SError("every length must be in 2..Tmax=%d (got %s); T = 1 gives an empty waveform" % (Tmax, frames))
    prm = params(hp)
    device = mels.device
    off_h, off = ragged.offsets(frames, device)
    total = int(off_h[-1])
    ws = workspace(lib.b2s_voc_ws_bytes(C.byref(prm), B, total, Tmax, WS_MEL2WAV), device)
    _, inv_t = _device_tables(hp, device)
    wav = torch.empty(B, int(hp.hop_length) * (Tmax - 1), dtype=torch.float32, device=device)
    check(lib.b2s_voc_mel2wav(C.byref(prm), ptr(mels), ptr(off), B, Tmax, total, n_iter, ptr(inv_t), ptr(wav), ptr(ws),
                              ws.numel(), stream(device)))
    return wav, [int(hp.hop_length) * (t - 1) for t in frames]


def wav2mel_batch(wavs, lengths, hp=None):
    """Normalised mels of a padded batch of waveforms [B, Lmax] (cuda tensor or NumPy) with per-utterance sample counts `lengths`
    (host sequence, every L_b >= 2).  Returns (mels [B, 1 + Lmax // hop, n_mels] cuda fp32, zero past each frame count,
    frame_lengths = 1 + L_b // hop)."""
    hp = default_hp(hp)
    lib = load()
    if isinstance(wavs, np.ndarray):
        wavs = torch.from_numpy(np.ascontiguousarray(wavs, dtype=np.float32)).cuda()
    if wavs.dim() != 2:
        raise B2SError("wavs must be [B, Lmax], got %s" % (tuple(wavs.shape),))
    if wavs.dtype != torch.float32:
        raise B2SError("wavs must be float32, got %s" % wavs.dtype)
    ptr(wavs)
    B, Lmax = int(wavs.shape[0]), int(wavs.shape[1])
    samples = [int(n) for n in lengths]
    if len(samples) != B:
        raise B2SError("%d lengths for a batch of %d" % (len(samples), B))
    if any(n < 2 or n > Lmax for n in samples):
        raise B2SError("every length must be in 2..Lmax=%d samples (got %s)" % (Lmax, samples))
    prm = params(hp)
    hop = int(hp.hop_length)
    device = wavs.device
    frames = [1 + n // hop for n in samples]
    off_h, off = ragged.offsets(frames, device)
    total = int(off_h[-1])
    Tout = 1 + Lmax // hop
    ws = workspace(lib.b2s_voc_ws_bytes(C.byref(prm), B, total, Tout, WS_WAV2MEL), device)
    basis, _ = _device_tables(hp, device)
    lens = torch.tensor(samples, dtype=torch.int32).to(device)
    mels = torch.zeros(B, Tout, int(hp.num_mels), dtype=torch.float32, device=device)
    check(lib.b2s_voc_wav2mel(C.byref(prm), ptr(wavs), ptr(lens), ptr(off), B, Lmax, total, ptr(basis), ptr(mels), ptr(ws),
                              ws.numel(), stream(device)))
    return mels, frames


# ---------------------------------------------------------------------------------------------------- silence splitting / trimming

def trim_params(hp=None):
    """(top_db, frame_length, hop_length) of the reference's trim_silence_intervals: 50 dB, 8 analysis windows, one frame shift."""
    hp = default_hp(hp)
    return 50, int(hp.sr / 1000 * hp.frame_length_ms) * 8, int(hp.sr / 1000 * hp.frame_shift_ms)


def _split_device(wavs, lengths, top_db, frame_length, hop_length, want_flags=False):
    """One b2s_voc_silence_split call.  Returns a dict of device tensors (intervals [B, NI, 2], n, trim [B, 2], prefix [B, NI],
    out_lengths [B], flags [B, Fmax] or None) plus the checked wavs tensor and the frame counts; nothing is synchronised."""
    lib = load()
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
    top_db, fl, hop = float(top_db), int(frame_length), int(hop_length)
    device = wavs.device
    ws = workspace(lib.b2s_voc_silence_ws_bytes(B, Lmax, fl, hop), device)
    frames = [1 + (n + 2 * (fl // 2) - fl) // hop for n in samples]
    fmax = 1 + (Lmax + 2 * (fl // 2) - fl) // hop
    ni = (fmax + 1) // 2
    lens = torch.tensor(samples, dtype=torch.int32).to(device)
    i32 = dict(dtype=torch.int32, device=device)
    out = {"intervals": torch.empty(B, ni, 2, **i32), "n": torch.empty(B, **i32), "trim": torch.empty(B, 2, **i32),
           "prefix": torch.empty(B, ni, **i32), "out_lengths": torch.empty(B, **i32),
           "flags": torch.empty(B, fmax, dtype=torch.uint8, device=device) if want_flags else None,
           "wavs": wavs, "frames": frames, "shape": (B, Lmax, fl, hop)}
    check(lib.b2s_voc_silence_split(ptr(wavs), ptr(lens), B, Lmax, top_db, fl, hop, ptr(out["intervals"]), ptr(out["n"]), ptr(out["trim"]),
                                    ptr(out["prefix"]), ptr(out["out_lengths"]), ptr(out["flags"]) if want_flags else None, ptr(ws),
                                    ws.numel(), stream(device)))
    return out


def _gather_device(sp):
    """b2s_voc_silence_gather on the result of _split_device: wav_out [B, Lmax] cuda fp32, zero past out_lengths."""
    B, Lmax, fl, hop = sp["shape"]
    wavs = sp["wavs"]
    wav_out = torch.empty_like(wavs)
    check(load().b2s_voc_silence_gather(ptr(wavs), B, Lmax, fl, hop, ptr(sp["intervals"]), ptr(sp["n"]), ptr(sp["prefix"]),
                                        ptr(sp["out_lengths"]), ptr(wav_out), stream(wavs.device)))
    return wav_out


def split_batch(wavs, lengths, top_db=60, frame_length=2048, hop_length=512, return_flags=False):
    """librosa.effects.split of every utterance of a padded batch [B, Lmax] (cuda tensor or NumPy) with per-utterance sample counts
    `lengths` (host sequence, every L_b >= 2): a list of int64 [n_b, 2] arrays of [start, end) sample indices.  With return_flags,
    also the list of per-frame non-silent flags (bool [F_b])."""
    sp = _split_device(wavs, lengths, top_db, frame_length, hop_length, want_flags=return_flags)
    n = sp["n"].cpu().numpy()
    iv = sp["intervals"].cpu().numpy()
    out = [iv[b, :n[b]].astype(np.int64) for b in range(len(n))]
    if return_flags:
        fl = sp["flags"].cpu().numpy()
        return out, [fl[b, :f].astype(bool) for b, f in enumerate(sp["frames"])]
    return out


def trim_batch(wavs, lengths, top_db=60, frame_length=2048, hop_length=512):
    """librosa.effects.trim's index of every utterance: int64 [B, 2] (start, end) with the kept signal y[start:end]."""
    return _split_device(wavs, lengths, top_db, frame_length, hop_length)["trim"].cpu().numpy().astype(np.int64)


def remove_silence_batch(wavs, lengths, top_db=60, frame_length=2048, hop_length=512):
    """np.concatenate([y[l:r] for l, r in librosa.effects.split(y, ...)]) for every utterance of a padded batch: (wav_out [B, Lmax]
    cuda fp32 with the non-silent intervals concatenated and zeros after, out_lengths as a list).  Kept samples are bit-equal to the
    input's.  Split and gather run on torch.cuda.current_stream(); reading out_lengths back is the only synchronisation."""
    sp = _split_device(wavs, lengths, top_db, frame_length, hop_length)
    wav_out = _gather_device(sp)
    return wav_out, [int(n) for n in sp["out_lengths"].cpu().numpy()]


def trim_silence_intervals_batch(wavs, lengths, hp=None):
    """The reference's trim_silence_intervals on a padded batch: remove_silence_batch with its parameters (trim_params)."""
    return remove_silence_batch(wavs, lengths, *trim_params(hp))


# ------------------------------------------------------------------------------------------------------ the reference's signatures

def _one_wav(y):
    y = np.asarray(y, dtype=np.float32)
    if y.ndim != 1:
        raise B2SError("wav must be 1-D, got %s" % (y.shape,))
    return y


def trim_silence_intervals(wav, hp=None):
    """The reference's utils.audio.trim_silence_intervals: waveform (NumPy) -> float32 waveform without its silent intervals."""
    wav = _one_wav(wav)
    out, lens = trim_silence_intervals_batch(wav[None], [wav.shape[0]], hp=hp)
    return out[0, :lens[0]].cpu().numpy()


def effects_split(y, top_db=60, frame_length=2048, hop_length=512):
    """librosa.effects.split(y, top_db, frame_length=..., hop_length=...) for a mono waveform: int64 [n, 2]."""
    y = _one_wav(y)
    return split_batch(y[None], [y.shape[0]], top_db, frame_length, hop_length)[0]


def effects_trim(y, top_db=60, frame_length=2048, hop_length=512):
    """librosa.effects.trim: (y[start:end], np.array([start, end]))."""
    y = _one_wav(y)
    idx = trim_batch(y[None], [y.shape[0]], top_db, frame_length, hop_length)[0]
    return y[idx[0]:idx[1]], idx


def mel2wav(mel, hp=None):
    """The reference's utils.audio.mel2wav: normalised mel [T, n_mels] (NumPy) -> float32 wav of hop * (T - 1) samples."""
    mel = np.asarray(mel, dtype=np.float32)
    if mel.ndim != 2:
        raise B2SError("mel must be [T, n_mels], got %s" % (mel.shape,))
    wav, lens = mel2wav_batch(mel[None], [mel.shape[0]], hp=hp)
    return wav[0, :lens[0]].cpu().numpy()


def get_spectrograms(wav, hp=None):
    """The reference's utils.audio.get_spectrograms: waveform (NumPy) -> normalised mel [1 + len // hop, n_mels] float32."""
    wav = np.asarray(wav, dtype=np.float32)
    if wav.ndim != 1:
        raise B2SError("wav must be 1-D, got %s" % (wav.shape,))
    mels, frames = wav2mel_batch(wav[None], [wav.shape[0]], hp=hp)
    return mels[0, :frames[0]].cpu().numpy()


def save_wav(wav, path, hp=None):
    """The reference's save_wav: peak-normalise by 1 / max(0.01, max|wav|) and write 16-bit PCM mono at hp.sr (what soundfile
    writes for .wav by default), through the stdlib `wave` module."""
    hp = default_hp(hp)
    wav = np.asarray(wav, dtype=np.float64).reshape(-1)
    scaled = wav / max(0.01, float(np.max(np.abs(wav))) if wav.size else 0.0)
    pcm = np.round(np.clip(scaled, -1.0, 1.0) * 32767).astype("<i2")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(hp.sr))
        w.writeframes(pcm.tobytes())
    return path
