"""Alignment-head selection and diagnostics on the GPU (b2s_met_align_* of libb2s_metrics.so, C ABI in include/b2s_metrics.h).

The reference's utils/infolog.py plot_attn receives every encoder-decoder attention map of an utterance (n_decoder_layer x
n_attention_head arrays of [dec, enc]), scores each by the sum over decoder steps of the per-step maximum, and draws the single best
one.  select_alignments runs that scoring where the maps already are, so that one map per utterance leaves the device, and adds
integer diagnostics of the chosen head's argmax path (backward steps, largest forward jump, encoder positions visited, last
position): a skipped or looping sample shows in them without a transcription.  plot_selected draws the reference's figure from the
selected map with matplotlib alone.  Opt-in through hp.align == "hip" (synthesize.eval_batch / save_eval_results); there is no CPU
fallback: a missing library is an error.
"""
import ctypes as C
import threading

import numpy as np
import torch

from . import metrics, ragged
from .cbind import B2SError, choice, dptr as p, stream

STAT_NAMES = ("backward_steps", "max_jump", "positions_visited", "last_position")
MAX_LAYERS = 16

_plot_lock = threading.Lock()          # one figure at a time, as in the reference (save_eval_results passes the reference's own lock)


def mode(hp=None):
    """hp.align, checked: "reference" or "hip"; anything else is a ValueError."""
    return choice(hp, "align")


def chunk():
    """Decoder frames per workgroup of the reduction kernel (scores are summed per chunk, then over the chunks in order)."""
    return int(metrics.load().b2s_met_align_chunk())


def select_alignments(encdec, input_lengths, generated_lengths, want_maps=True):
    """encdec: list of 1..16 [B, H, S, T] fp32 arrays or tensors (any device), one per decoder layer, T innermost -- eval_batch's
    alignments['encdec'].  Lengths: lists, arrays or tensors; clamped to [0, S] and [0, T] on the device.

    Returns device tensors, queued on the current stream without synchronising: `scores` [B, L, H] float64 (sum over t < dec_len of
    max over s < enc_len), `layer` / `head` [B] int32 of the largest score (strict >, the first wins a tie; -1 when no score is > 0,
    e.g. dec_len 0), `focus` [B] float64 = best score / max(dec_len, 1), `paths` [B, T] int32 (the chosen head's argmax per frame, -1
    past dec_len), `stats` [B, 4] int32 (STAT_NAMES) and, with want_maps, `maps` [B, S, T] float32: the chosen head's slab unchanged
    (zeros without a choice)."""
    mode()                                             # an unknown hp.align is refused wherever the feature is reached
    lib = metrics.load()
    encdec = list(encdec)
    if not 1 <= len(encdec) <= MAX_LAYERS:
        raise B2SError("select_alignments takes 1..%d layers (got %d)" % (MAX_LAYERS, len(encdec)))
    device = ragged.device("the DTW metric", encdec[0])
    layers = []
    for a in encdec:
        t = ragged.as_tensor(a)
        if t.dim() != 4 or (layers and t.shape != layers[0].shape):
            raise B2SError("every layer must be [B, H, S, T] of one shape (got %s)" % (tuple(t.shape),))
        layers.append(t.to(device=device, dtype=torch.float32).contiguous())
    B, H, S, T = (int(v) for v in layers[0].shape)
    L = len(layers)
    nbytes = lib.b2s_met_align_ws_bytes(B, L, H, S, T)
    ws = metrics.workspace(nbytes, device)
    enc = ragged.lengths_i32(input_lengths, B, device, "input_lengths")
    dec = ragged.lengths_i32(generated_lengths, B, device, "generated_lengths")
    scores = torch.empty(B, L, H, dtype=torch.float64, device=device)
    best = torch.empty(B, dtype=torch.int32, device=device)
    maps = torch.empty(B, S, T, dtype=torch.float32, device=device) if want_maps else None
    paths = torch.empty(B, T, dtype=torch.int32, device=device)
    stats = torch.empty(B, 4, dtype=torch.int32, device=device)
    table = (C.c_void_p * L)(*[t.data_ptr() for t in layers])          # host array: the pointers travel in the kernel arguments
    with torch.cuda.device(device):
        metrics.check(lib.b2s_met_align_select(C.cast(table, C.c_void_p), L, B, H, S, T, p(enc), p(dec), p(scores), p(best), p(maps),
                                               p(paths), p(stats), p(ws), nbytes, stream(device)))
    has = best >= 0
    safe = best.clamp(min=0).to(torch.int64)
    top = scores.reshape(B, L * H).gather(1, safe.unsqueeze(1)).squeeze(1)
    none = torch.full_like(best, -1)
    out = {"scores": scores,
           "layer": torch.where(has, torch.div(best, H, rounding_mode="floor"), none),
           "head": torch.where(has, best % H, none),
           "focus": torch.where(has, top, torch.zeros_like(top)) / dec.clamp(min=1, max=T).to(torch.float64),
           "paths": paths, "stats": stats}
    if want_maps:
        out["maps"] = maps
    return out


def summary(selected, i):
    """Plain-Python diagnostics of sample i from eval_batch's alignments['selected'] (what `<name>_align.json` holds)."""
    layer, head = int(selected["layer"][i]), int(selected["head"][i])
    scores = np.asarray(selected["scores"][i]) if not isinstance(selected["scores"], torch.Tensor) else selected["scores"][i].cpu().numpy()
    out = {"layer": layer, "head": head, "score": float(scores[layer, head]) if layer >= 0 else 0.0,
           "focus": float(selected["focus"][i])}
    for k, name in enumerate(STAT_NAMES):
        out[name] = int(selected["stats"][i][k])
    return out


def plot_selected(map_ts, info, path, lock=None):
    """The reference's alignment figure (utils/infolog.py plot_attn) for an already selected head: map_ts is its [dec, enc] crop,
    info a dict with `layer` and `head` (or the title itself).  Needs matplotlib only.

    The figure is built through matplotlib's object interface on an Agg canvas of its own: pyplot's process-wide current figure is
    never touched, so a pyplot user in another thread (the reference's plot_mel) cannot draw into this figure, nor this call into
    theirs.  One figure is drawn at a time under `lock`; pass the lock of the other plotting code of the process (the reference's
    utils.infolog.lock) to share it, the default is the module's own."""
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from matplotlib.figure import Figure
    title = info if isinstance(info, str) else "Layer %d, Head %d" % (info["layer"], info["head"])
    with (_plot_lock if lock is None else lock):
        fig = Figure(figsize=(14, 7))
        FigureCanvasAgg(fig)
        ax = fig.add_subplot()
        ax.pcolor(np.asarray(map_ts))
        ax.set_title(title)
        fig.savefig(path)
