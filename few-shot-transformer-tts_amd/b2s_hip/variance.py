"""ctypes binding of libb2s_va.so (C ABI in include/b2s_va.h): the variance adaptor of a FastSpeech-2-style student on the GPU,
forward and backward.

b2s_hip.durations and b2s_hip.prosody extract a duration, a pitch and an energy per input unit; this module is what consumes them
(DESIGN.md section o).  quantise_batch turns pitch or energy into bins, expand adds one embedding row per bin to the encoder output
of each position and repeats the sum for as many frames as the position's duration (the length regulator), and its backward is the
transposed operation: a sum over each position's frames and a sum of the position gradients into the embedding tables, without
atomics.  Every fp32 sum is made in a fixed order, so the results repeat bit for bit, for an utterance alone or inside a batch.
There is no CPU fallback.

    va = VarianceAdaptor(256, 768, boundaries_from_stats(stats, "pitch", 256), boundaries_from_stats(stats, "energy", 256)).cuda()
    out = va(encoder_output, pitch, energy, durations, input_lengths, frame_lengths=mel_lengths)
    decoder_input = padded(out["frames"], out["frame_offsets"], T)
"""
import ctypes as C
import json
import math

import numpy as np
import torch

from . import ragged
from .cbind import EMPTY, FAILED, OK  # noqa: F401 (the status words are part of this module's surface)
from .cbind import B2SError, Library, dptr, nptr, raise_failed, stream
from .ragged import as_tensor, lengths_i32

STATUS_NAMES = ("OK", "EMPTY", "FAILED")
MAX_S, MAX_D, MAX_BINS, MAX_FRAMES = 1024, 1024, 256, 1 << 20

P = C.c_void_p
_I = C.c_int
_PROTOS = {
    "b2s_va_version": (C.c_int, []),
    "b2s_va_last_error": (C.c_char_p, []),
    "b2s_va_ws_bytes": (C.c_size_t, [_I, _I, _I, _I]),
    "b2s_va_quantise": (C.c_int, [P, P, P, _I, _I, _I, P, P, P]),
    "b2s_va_frames": (C.c_int, [P, P, _I, _I, P, P, P]),
    "b2s_va_forward": (C.c_int, [P, P, P, P, P, _I, P, P, P, _I, _I, _I, _I, P, P, P, P, P]),
    "b2s_va_backward": (C.c_int, [P, P, P, _I, P, P, P, _I, _I, _I, _I, P, P, P, P, P, C.c_size_t, P]),
    "b2s_va_pad": (C.c_int, [P, P, _I, _I, _I, _I, P, _I, P, P]),
}
_LIB = Library("libb2s_va.so", _PROTOS, "b2s_va_last_error")
LIB_PATH, EXPORTS, load, check, workspace = _LIB.path, _LIB.exports, _LIB.load, _LIB.check, _LIB.workspace


def _device(*arrays):
    return ragged.device("the variance adaptor", *arrays)


def _int_batch(a, device, what):
    t = as_tensor(a)
    if t.dim() != 2:
        raise B2SError("%s must be [B, S], got %s" % (what, tuple(t.shape)))
    return t.to(device=device, dtype=torch.int32).contiguous()


# --------------------------------------------------------------------------------------------------------- quantise and frames

def quantise_batch(values, input_lengths, boundaries):
    """b2s_va_quantise: values [B, S] (any float type, compared in fp64) with input_lengths [B] and boundaries [n_bins - 1], finite
    and strictly ascending.  Returns device tensors (bins [B, S] int32, status [B] int32): bins = the count of boundaries strictly
    below the value (torch.bucketize(right=False)), 0 from input_lengths on.  Nothing is raised and nothing is read back."""
    lib = load()
    device = _device(values, boundaries)
    v = as_tensor(values)
    if v.dim() != 2:
        raise B2SError("values must be [B, S], got %s" % (tuple(v.shape),))
    v = v.to(device=device, dtype=torch.float64).contiguous()
    bd = as_tensor(boundaries).reshape(-1).to(device=device, dtype=torch.float64).contiguous()
    B, S = int(v.shape[0]), int(v.shape[1])
    n_in = lengths_i32(input_lengths, B, device, "input_lengths")
    bins = torch.empty(B, S, dtype=torch.int32, device=device)
    status = torch.empty(B, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        check(lib.b2s_va_quantise(nptr(v), nptr(n_in), nptr(bd), int(bd.numel()) + 1, B, S, nptr(bins), nptr(status), stream(device)))
    return bins, status


def frame_counts(durations, input_lengths):
    """b2s_va_frames: durations [B, S] integers with input_lengths [B] -> device tensors (frames [B] int32, status [B] int32)."""
    lib = load()
    device = _device(durations)
    d = _int_batch(durations, device, "durations")
    B, S = int(d.shape[0]), int(d.shape[1])
    n_in = lengths_i32(input_lengths, B, device, "input_lengths")
    frames = torch.empty(B, dtype=torch.int32, device=device)
    status = torch.empty(B, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        check(lib.b2s_va_frames(nptr(d), nptr(n_in), B, S, nptr(frames), nptr(status), stream(device)))
    return frames, status


# ---------------------------------------------------------------------------------------------------------------------- expand

class _Expand(torch.autograd.Function):
    """b2s_va_forward, and b2s_va_backward as its backward.  The index tensors are device int32, contiguous."""

    @staticmethod
    def forward(ctx, x, pitch_table, energy_table, pb, eb, dur, n_in, off, total):
        lib = load()
        device = x.device
        B, S, D = (int(v) for v in x.shape)
        tables = [t for t in (pitch_table, energy_table) if t is not None]
        n_bins = int(tables[0].shape[0]) if tables else 1
        y = torch.empty(total, D, dtype=torch.float32, device=device)
        uof = torch.empty(total, dtype=torch.int32, device=device)
        status = torch.empty(B, dtype=torch.int32, device=device)
        x = x.contiguous()
        pt = None if pitch_table is None else pitch_table.contiguous()
        et = None if energy_table is None else energy_table.contiguous()
        with torch.cuda.device(device):
            check(lib.b2s_va_forward(nptr(x), dptr(pb), dptr(eb), dptr(pt), dptr(et), n_bins, nptr(dur), nptr(n_in), nptr(off), total,
                                     B, S, D, None, nptr(y), nptr(uof), nptr(status), stream(device)))
        ctx.save_for_backward(pb, eb, dur, n_in, off)
        ctx.sizes = (B, S, D, n_bins, total)
        ctx.mark_non_differentiable(uof, status)
        return y, uof, status

    @staticmethod
    def backward(ctx, dy, _duof, _dstatus):
        lib = load()
        pb, eb, dur, n_in, off = ctx.saved_tensors
        B, S, D, n_bins, total = ctx.sizes
        device = dy.device
        dy = dy.contiguous()
        need_p = pb is not None and ctx.needs_input_grad[1]
        need_e = eb is not None and ctx.needs_input_grad[2]
        dx = torch.empty(B, S, D, dtype=torch.float32, device=device)
        dpt = torch.empty(n_bins, D, dtype=torch.float32, device=device) if need_p else None
        det = torch.empty(n_bins, D, dtype=torch.float32, device=device) if need_e else None
        status = torch.empty(B, dtype=torch.int32, device=device)
        nbytes = lib.b2s_va_ws_bytes(B, S, D, n_bins)
        ws = workspace(nbytes, device)
        with torch.cuda.device(device):
            check(lib.b2s_va_backward(nptr(dy), dptr(pb), dptr(eb), n_bins, nptr(dur), nptr(n_in), nptr(off), total, B, S, D, nptr(dx),
                                      dptr(dpt), dptr(det), nptr(status), dptr(ws), nbytes, stream(device)))
        return dx, dpt, det, None, None, None, None, None, None


def _bins_and_table(pair, name, d_shape, D, device):
    if pair is None:
        return None, None
    bins, table = pair
    bins = _int_batch(bins, device, name + " bins")
    if tuple(bins.shape) != d_shape:
        raise B2SError("%s bins must have the shape of the durations %s (got %s)" % (name, d_shape, tuple(bins.shape)))
    if not isinstance(table, torch.Tensor) or table.dim() != 2 or int(table.shape[1]) != D or table.dtype != torch.float32:
        raise B2SError("the %s table must be an fp32 tensor [n_bins, %d]" % (name, D))
    if table.device != device:
        raise B2SError("the %s table is on %s, x on %s" % (name, table.device, device))
    return bins, table


def expand(x, durations, input_lengths, pitch=None, energy=None, frame_lengths=None, check_status=True):
    """Embed and expand: x [B, S, D] fp32 on the GPU, durations [B, S] integers, input_lengths [B]; pitch and energy are each None or
    a pair (bins [B, S], table [n_bins, D] fp32), and a term that is None is not added at all.  frame_lengths: the frames per
    utterance as host integers when they are known (the mel lengths, in training); None computes them with frame_counts and reads
    them back, the one host read of the call.  Differentiable in x and the tables (b2s_va_backward).

    Returns a dict: frames [total, D] fp32 packed by frame_offsets (host array [B + 1], frame_offsets_device its copy),
    frame_lengths (host list), unit_of_frame [total] int32 and status [B] int32.  check_status reads the status words and raises
    B2SError for a FAILED utterance (cbind.raise_failed); False leaves the words to the caller and reads nothing."""
    device = _device(x)
    if not isinstance(x, torch.Tensor):
        x = as_tensor(x).to(device=device, dtype=torch.float32)
    if x.dim() != 3 or x.dtype != torch.float32 or not x.is_cuda:
        raise B2SError("x must be an fp32 tensor [B, S, D] on the GPU, got %s %s" % (x.dtype, tuple(x.shape)))
    B, S, D = (int(v) for v in x.shape)
    dur = _int_batch(durations, device, "durations")
    if tuple(dur.shape) != (B, S):
        raise B2SError("durations must be [%d, %d], got %s" % (B, S, tuple(dur.shape)))
    n_in = lengths_i32(input_lengths, B, device, "input_lengths")
    pb, pt = _bins_and_table(pitch, "pitch", (B, S), D, device)
    eb, et = _bins_and_table(energy, "energy", (B, S), D, device)
    if pt is not None and et is not None and pt.shape != et.shape:
        raise B2SError("the two tables must have the same shape (got %s and %s)" % (tuple(pt.shape), tuple(et.shape)))
    if frame_lengths is None:
        frame_lengths = frame_counts(dur, n_in)[0].cpu().tolist()
    else:
        frame_lengths = ragged.lengths(frame_lengths, B, MAX_FRAMES, "frame_lengths")
    off_h, off = ragged.offsets(frame_lengths, device)
    y, uof, status = _Expand.apply(x, pt, et, pb, eb, dur, n_in, off, int(off_h[-1]))
    if check_status:
        raise_failed(status, "the variance adaptor", "utterances",
                     "a length, duration or bin outside its range, or durations that do not sum to frame_lengths")
    return {"frames": y, "frame_offsets": off_h, "frame_offsets_device": off, "frame_lengths": list(frame_lengths),
            "unit_of_frame": uof, "status": status}


def _pad(frames, off, padded_block, to_frames):
    lib = load()
    device = padded_block.device
    B, T, D = (int(v) for v in padded_block.shape)
    status = torch.empty(B, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        check(lib.b2s_va_pad(nptr(frames), nptr(off), int(frames.shape[0]), B, T, D, nptr(padded_block), int(to_frames), nptr(status),
                             stream(device)))


class _Padded(torch.autograd.Function):
    """b2s_va_pad, and the same call in the other direction as its backward.  The host has checked the offsets against T."""

    @staticmethod
    def forward(ctx, frames, off, T):
        frames = frames.contiguous()
        out = torch.empty(int(off.numel()) - 1, T, int(frames.shape[1]), dtype=torch.float32, device=frames.device)
        _pad(frames, off, out, False)
        ctx.save_for_backward(off)
        ctx.total = int(frames.shape[0])
        return out

    @staticmethod
    def backward(ctx, d_out):
        off, = ctx.saved_tensors
        d_out = d_out.contiguous()
        d_frames = torch.empty(ctx.total, int(d_out.shape[2]), dtype=torch.float32, device=d_out.device)
        _pad(d_frames, off, d_out, True)
        return d_frames, None, None


def padded(frames, frame_offsets, T):
    """Packed frames [total, D] (fp32, on the GPU) with their B + 1 host offsets -> [B, T, D] with zeros behind each utterance
    (b2s_va_pad; differentiable, the backward is the same call in the other direction)."""
    off = np.asarray(frame_offsets, dtype=np.int64).reshape(-1)
    lens = off[1:] - off[:-1]
    if not isinstance(frames, torch.Tensor) or frames.dim() != 2 or frames.dtype != torch.float32:
        raise B2SError("frames must be an fp32 tensor [total, D]")
    if len(off) < 2 or off[0] != 0 or (lens < 0).any() or int(off[-1]) != int(frames.shape[0]):
        raise B2SError("frame_offsets %s do not pack %d frames" % (off.tolist(), int(frames.shape[0])))
    if (lens > T).any():
        raise B2SError("an utterance of %d frames does not fit T = %d" % (int(lens.max()), T))
    device = _device(frames)
    if not frames.is_cuda:
        raise B2SError("frames must be on the GPU (they are on %s)" % frames.device)
    return _Padded.apply(frames, torch.from_numpy(off.astype(np.int32)).to(device), int(T))


# ---------------------------------------------------------------------------------------------------------------- the module

def boundaries_from_stats(stats, key, n_bins, scale="linear"):
    """The n_bins - 1 boundaries of n_bins bins of equal width between the overall minimum and maximum of `key` ("pitch", "energy",
    ..) in prosody's stats.json (a dict, or the path of the file); scale="log": of equal width in the logarithm, which needs a
    minimum above 0.  Host only.  Returns fp64 [n_bins - 1]; a statistic over 0 units is refused."""
    if isinstance(stats, str):
        with open(stats, encoding="utf-8") as f:
            stats = json.load(f)
    if scale not in ("linear", "log"):
        raise B2SError("unknown scale %r (expected 'linear' or 'log')" % (scale,))
    if not 1 <= int(n_bins) <= MAX_BINS:
        raise B2SError("n_bins must be in 1..%d (got %d)" % (MAX_BINS, n_bins))
    try:
        st = stats["overall"][key]
    except (KeyError, TypeError):
        raise B2SError("the statistics have no overall %r" % (key,))
    if not st.get("count"):
        raise B2SError("the statistics of %r are over 0 units: no boundaries" % (key,))
    lo, hi = float(st["min"]), float(st["max"])
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise B2SError("min and max of %r must be finite (got %r and %r)" % (key, lo, hi))
    if scale == "log":
        if lo <= 0.0:
            raise B2SError("a log scale needs a minimum above 0 (%r has %r)" % (key, lo))
        lo, hi = math.log(lo), math.log(hi)
    edges = np.linspace(lo, hi, int(n_bins) + 1, dtype=np.float64)[1:-1]
    edges = np.exp(edges) if scale == "log" else edges
    if len(edges) and not np.all(edges[1:] > edges[:-1]) or (n_bins > 1 and not hi > lo):
        raise B2SError("%d bins between %r and %r do not ascend strictly" % (n_bins, st["min"], st["max"]))
    return edges


class VarianceAdaptor(torch.nn.Module):
    """Quantise pitch and energy, add their embeddings to the encoder output and expand by the durations.  Parameters
    pitch_embedding.weight and energy_embedding.weight [n_bins, D] fp32; buffers pitch_boundaries and energy_boundaries [n_bins - 1]
    fp64 (boundaries_from_stats)."""

    def __init__(self, n_bins, dim, pitch_boundaries, energy_boundaries):
        super(VarianceAdaptor, self).__init__()
        if not 1 <= n_bins <= MAX_BINS:
            raise B2SError("n_bins must be in 1..%d (got %d)" % (MAX_BINS, n_bins))
        if dim < 4 or dim > MAX_D or dim % 4:
            raise B2SError("D must be a multiple of 4 in 4..%d (got %d)" % (MAX_D, dim))
        self.n_bins, self.dim = int(n_bins), int(dim)
        self.pitch_embedding = torch.nn.Embedding(n_bins, dim)
        self.energy_embedding = torch.nn.Embedding(n_bins, dim)
        for name, bd in (("pitch_boundaries", pitch_boundaries), ("energy_boundaries", energy_boundaries)):
            t = as_tensor(bd).reshape(-1).to(torch.float64).clone()
            if int(t.numel()) != n_bins - 1:
                raise B2SError("%s: %d boundaries for %d bins" % (name, int(t.numel()), n_bins))
            self.register_buffer(name, t)

    def forward(self, x, pitch, energy, durations, input_lengths, frame_lengths=None, check_status=True):
        """x [B, S, D], pitch and energy [B, S] (prosody's targets), durations [B, S], input_lengths [B] -> the dict of expand, with
        `pitch_bins` and `energy_bins` added; an utterance whose pitch or energy holds a NaN is FAILED."""
        pb, ps = quantise_batch(pitch, input_lengths, self.pitch_boundaries)
        eb, es = quantise_batch(energy, input_lengths, self.energy_boundaries)
        out = expand(x, durations, input_lengths, (pb, self.pitch_embedding.weight), (eb, self.energy_embedding.weight),
                     frame_lengths, check_status=False)
        out["status"] = torch.maximum(out["status"], torch.maximum(ps, es))
        out["pitch_bins"], out["energy_bins"] = pb, eb
        if check_status:
            raise_failed(out["status"], "the variance adaptor", "utterances",
                         "a NaN target, a length, duration or bin outside its range, or durations that do not sum to frame_lengths")
        return out
