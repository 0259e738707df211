"""NumPy restatements for the alignment-head selection (b2s_hip.alignment, b2s_met_align_select).

(a) select(): the contract of include/b2s_metrics.h in fp64 -- scores, the chosen head, its map, the argmax path and its statistics.
(b) plot_attn_choice(): the selection rule of the reference's utils/infolog.py plot_attn with its arithmetic: layers of
    [heads, dec, enc] arrays cropped by the lengths (only when a length is truthy), the per-step maxima of each head added one by
    one into a running NumPy-fp32 sum, strict > against a running best that starts at 0.  Restated, not copied.

make_case() is the seeded generator of the GPU tests: softmax over s of random logits with a distinct sharpness per (layer, head),
and every position past a length overwritten with 7.0 afterwards, so that a read past a length changes the answer.
"""
import numpy as np


def select(layers, enc_len, dec_len):
    """layers: list of [B, H, S, T] fp32 arrays.  Returns a dict of scores [B, L, H] f64, best [B] (l * H + h, -1 for none),
    maps [B, S, T] f32, paths [B, T] int32 (-1 past dec_len or without a choice) and stats [B, 4] int32."""
    L = len(layers)
    B, H, S, T = layers[0].shape
    scores = np.zeros((B, L, H), np.float64)
    best = np.full(B, -1, np.int32)
    maps = np.zeros((B, S, T), np.float32)
    paths = np.full((B, T), -1, np.int32)
    stats = np.zeros((B, 4), np.int32)
    for b in range(B):
        e, d = min(max(int(enc_len[b]), 0), S), min(max(int(dec_len[b]), 0), T)
        if e > 0 and d > 0:
            for l in range(L):
                scores[b, l] = layers[l][b, :, :e, :d].max(axis=1).astype(np.float64).sum(axis=1)
        best_v = 0.0
        for l in range(L):
            for h in range(H):
                if scores[b, l, h] > best_v:
                    best_v, best[b] = scores[b, l, h], l * H + h
        if best[b] < 0:
            continue
        chosen = layers[best[b] // H][b, best[b] % H]
        maps[b] = chosen
        p = chosen[:e, :d].argmax(axis=0).astype(np.int32)
        paths[b, :d] = p
        step = np.diff(p.astype(np.int64))
        stats[b] = [int((step < 0).sum()), int(max(step.max(), 0)) if len(step) else 0, len(np.unique(p)), int(p[-1])]
    return {"scores": scores, "best": best, "maps": maps, "paths": paths, "stats": stats}


def plot_attn_choice(attn, enc_length=None, dec_length=None):
    """attn: list over layers of [heads, dec, enc] arrays, as save_eval_results hands them to plot_attn.  Returns
    (layer, head, the [dec, enc] crop that would be drawn), or (-1, -1, None) when no head scores above 0."""
    chosen, top = (-1, -1, None), 0
    for li, maps in enumerate(attn):
        crop = np.asarray(maps)
        crop = crop[:, :dec_length or None, :enc_length or None]          # a length of 0 (or None) crops nothing there
        maxima = crop.max(axis=2)                                         # [heads, dec], exact in the input's fp32
        for hi in range(crop.shape[0]):
            total = 0                                                     # the int 0, then a NumPy float32 running sum, step by step
            for v in maxima[hi]:
                total = total + v
            if total > top:                                               # strict: the first of equal heads stays
                chosen, top = (li, hi, crop[hi]), total
    return chosen


def sharpness_ladder(L, H):
    """A distinct softmax sharpness (the standard deviation of the logits) per (layer, head), evenly spaced in 0.3..3.3 with the
    sharpest one in the middle of the scan order, so that neither `first` nor `last` is the answer.  The top of the ladder stays
    well short of a one-hot softmax: saturated heads would all score dec_len and leave no gap between the best two."""
    n = L * H
    order = np.roll(np.arange(n), n // 2 + 1)
    return (0.3 + 3.0 * order / max(n - 1, 1)).reshape(L, H)


def make_case(seed, B, L, H, S, T, enc_len, dec_len):
    """Seeded list of L [B, H, S, T] fp32 layers: softmax over all S positions, then 7.0 past either length."""
    rng = np.random.default_rng(seed)
    sharp = sharpness_ladder(L, H)
    layers = []
    for l in range(L):
        logits = rng.standard_normal((B, H, S, T)) * sharp[l][None, :, None, None]
        a = np.exp(logits - logits.max(axis=2, keepdims=True))
        a = (a / a.sum(axis=2, keepdims=True)).astype(np.float32)
        for b in range(B):
            a[b, :, min(int(enc_len[b]), S):, :] = 7.0
            a[b, :, :, min(int(dec_len[b]), T):] = 7.0
        layers.append(a)
    return layers


def duplicate_best(layers, best):
    """Make an exact tie for every utterance with a choice: its best head's slab is copied over head 0 of layer 0 (earlier in the
    scan order, so that one must win), or, where the best head is that one already, over the last head of the last layer.
    Returns the expected choice per utterance."""
    H = layers[0].shape[1]
    want = np.array(best).copy()
    for b, k in enumerate(best):
        if k > 0:
            layers[0][b, 0] = layers[k // H][b, k % H]
            want[b] = 0
        elif k == 0:
            layers[-1][b, H - 1] = layers[0][b, 0]
    return want


SEED = 5


def gpu_cases(chunk):
    """name -> (B, L, H, S, T, enc_len, dec_len) of the GPU tests; `chunk` is the kernel's frames per workgroup."""
    return {
        "ragged": (4, 2, 3, 37, 70, [37, 20, 1, 5], [70, 33, 1, 0]),
        # T beyond one chunk, neither a multiple of it nor of 4 (dword loads); a dec_len inside the second chunk
        "two_chunks_odd": (2, 1, 2, 130, chunk + 3, [130, 77], [chunk + 3, chunk + 1]),
        # T a multiple of 4 (16-byte loads) with dec_len ending inside a lane's four frames, and a whole chunk past dec_len
        "two_chunks_vec": (2, 2, 2, 21, chunk + 8, [21, 9], [chunk + 6, chunk - 3]),
        # the 16-byte path's eight-rows-in-flight loop: T a multiple of 4 and 38 / 36 (enc 150) and 17 / 16 (enc 67) rows per wave,
        # i.e. 4 and 2 unrolled passes with a remainder of 6 / 4 / 1 / 0 rows; dec_len ends inside a lane's four frames
        "two_chunks_vec_deep": (2, 2, 2, 150, chunk + 8, [150, 67], [chunk + 6, chunk - 3]),
        "sixteen_layers": (3, 16, 1, 19, 41, [19, 8, 13], [41, 17, 40]),
    }


def best_gap(scores_b):
    """fp64 gap between the largest and the second-largest score of one utterance ([L, H])."""
    s = np.sort(scores_b.reshape(-1))
    return float(s[-1] - s[-2]) if len(s) > 1 else float(s[-1])
