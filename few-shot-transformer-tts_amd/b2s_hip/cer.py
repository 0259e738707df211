"""Character error rate of the eval on the GPU: batched edit distance (b2s_met_edit_* of libb2s_metrics.so, C ABI in
include/b2s_metrics.h), the reference's text normalisation and CER formula, and the per-locale summary of a transcriptions.jsonl.

The reference's utils/transcribe.py scores a transcription as min(1.0, editdistance.eval(truth, pred) / (len(pred) + 1e-9)) after
basic_normalize on both texts, and eval.run_transcription averages the scores per locale.  The speech recogniser stays external;
everything after it is here, without the editdistance package:

    basic_normalize(text, locale)            the reference's normalisation (unicodedata + re, on the host)
    edit_distance_batch(truths, preds)       Levenshtein distances of B pairs in one launch, optionally with the exact breakdown into
                                             substitutions, deletions and insertions; items are str (code points), bytes, integer
                                             arrays, or lists of str tokens (word ids from one dict per call: WER on the same kernel)
    cer_batch(truths, preds)                 the reference's score per pair, bit-identical Python floats
    eval(a, b)                               editdistance.eval's call shape
    score_transcriptions(records_or_path)    re-scores a transcriptions.jsonl: raw CER, and per locale the mean CER that the eval's
                                             `cer` window reports, the micro-averaged CER and the summed error breakdown
    python -m b2s_hip.cer PATH/transcriptions.jsonl [--renormalize] [--json OUT]

install(hp) binds the `editdistance` global of the reference's utils.transcribe (if imported) to this module for hp.cer == "hip" and
restores it for "reference"; synthesize.eval_batch calls it.  There is no CPU fallback: a missing library or device is an error.
"""
import json
import logging
import os
import re
import sys
import types
import unicodedata

import numpy as np
import torch

from . import metrics, ragged, rescore
from .cbind import B2SError, choice, dptr as p, rebind, stream

OP_NAMES = ("sub", "del", "ins")

_DROPPED = frozenset(("Pc", "Pd", "Ps", "Pe", "Pi", "Pf", "Po"))                  # every punctuation category
_NO_SPACE_LOCALES = frozenset(("zh", "zh-cn", "th-th", "zh-tw", "zh-hk", "ja-jp", "ko-kr"))
_WHITESPACE = re.compile(r"\s+")


def basic_normalize(text, locale):
    """The reference's utils.transcribe.basic_normalize: punctuation dropped, spaces dropped for the locales written without them,
    lower case per character, whitespace runs to one space, NFD, stripped."""
    no_space = locale in _NO_SPACE_LOCALES
    kept = "".join(ch.lower() for ch in text
                   if unicodedata.category(ch) not in _DROPPED and not (no_space and ch == " "))
    return unicodedata.normalize("NFD", _WHITESPACE.sub(" ", kept)).strip()


def max_len():
    """Symbols per side that the kernel takes (4096)."""
    return int(metrics.load().b2s_met_edit_max_len())


# --------------------------------------------------------------------------------------------------------------- ragged batches

class Packed(object):
    """One side of a batch on the device: `symbols` int32 [total] (at least one element), `offsets` int32 [B + 1] on the host and
    `offsets_d` on the device, `lengths` (Python ints) and `max_len`.  pack() builds it; edit_distance_batch takes it as is."""

    def __init__(self, symbols, offsets, offsets_d):
        self.symbols, self.offsets, self.offsets_d = symbols, offsets, offsets_d
        self.lengths = [int(n) for n in np.diff(offsets)]
        self.max_len = max(self.lengths) if self.lengths else 0

    def __len__(self):
        return len(self.lengths)


def _symbols(item, vocab):
    if isinstance(item, str):
        return np.frombuffer(item.encode("utf-32-le", "surrogatepass"), dtype="<i4")
    if isinstance(item, (bytes, bytearray)):
        return np.frombuffer(bytes(item), dtype=np.uint8).astype(np.int32)
    if isinstance(item, torch.Tensor):
        item = item.detach().cpu().numpy()
    elif isinstance(item, (list, tuple)) and item and all(isinstance(t, str) for t in item):
        return np.asarray([vocab.setdefault(t, len(vocab)) for t in item], dtype=np.int32)
    arr = np.asarray(item)
    if arr.size == 0:
        return np.zeros(0, dtype=np.int32)
    if arr.ndim != 1 or arr.dtype.kind not in "iu":
        raise B2SError("a sequence must be a str, bytes, a 1-D integer array or a list of str tokens (got %s %s)"
                       % (arr.dtype, arr.shape))
    if arr.dtype != np.int32 and (arr.min() < -2 ** 31 or arr.max() >= 2 ** 31):
        raise B2SError("symbols must fit int32")
    return arr.astype(np.int32)


def pack(items, device=None, vocab=None):
    """Host sequences -> Packed on `device` (default: the current HIP device).  `vocab` is the token -> id dict that lists of str
    tokens share; pass the same dict for both sides of a comparison."""
    if device is None:
        device = ragged.device("the edit distance")
    vocab = {} if vocab is None else vocab
    parts = [_symbols(it, vocab) for it in items]
    off = ragged.offsets([len(part) for part in parts])
    flat = np.concatenate(parts) if off[-1] else np.zeros(1, dtype=np.int32)
    return Packed(torch.from_numpy(np.ascontiguousarray(flat, dtype=np.int32)).to(device), off, torch.from_numpy(off).to(device))


def _pack_both(truths, preds):
    vocab = {}
    a = truths if isinstance(truths, Packed) else pack(truths, vocab=vocab)
    b = preds if isinstance(preds, Packed) else pack(preds, vocab=vocab)
    if len(a) != len(b):
        raise B2SError("%d truths for %d predictions" % (len(a), len(b)))
    return a, b


def _run(a, b, return_ops):
    lib = metrics.load()
    limit = int(lib.b2s_met_edit_max_len())
    if a.max_len > limit or b.max_len > limit:
        raise B2SError("a sequence of %d symbols: the edit distance takes at most %d per side" % (max(a.max_len, b.max_len), limit))
    device = a.symbols.device
    n = len(a)
    dist = torch.empty(n, dtype=torch.int32, device=device)
    ops = torch.empty(n, 3, dtype=torch.int32, device=device) if return_ops else None
    if n == 0:
        return dist, ops
    status = torch.empty(n, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        metrics.check(lib.b2s_met_edit_distance(p(a.symbols), p(a.offsets_d), int(a.offsets[-1]), a.max_len, p(b.symbols),
                                                p(b.offsets_d), int(b.offsets[-1]), b.max_len, n, p(dist), p(ops), p(status), stream(device)))
    failed = torch.nonzero(status != metrics.OK).reshape(-1)
    if failed.numel():
        raise B2SError("edit distance failed for pairs %s (offsets inconsistent with the sizes)" % failed.cpu().tolist())
    return dist, ops


def edit_distance_batch(truths, preds, return_ops=False):
    """Levenshtein distance (unit costs) of every pair.  truths / preds: sequences of str (compared by code point), bytes, 1-D integer
    arrays or lists of str tokens, or Packed batches already on the device.  Returns a device int32 tensor [B], and with return_ops
    also [B, 3]: substitutions, deletions (truth symbols missing from the prediction) and insertions of the alignment with the fewest
    substitutions among the cheapest.  B2SError for a side longer than max_len() and for any pair the kernel refuses."""
    a, b = _pack_both(truths, preds)
    dist, ops = _run(a, b, return_ops)
    return (dist, ops) if return_ops else dist


def _score(d, n_pred):
    return min(1.0, d / (n_pred + 1e-9))


def _to_list(t):
    return t.cpu().tolist() if isinstance(t, torch.Tensor) else np.asarray(t).tolist()


def cer_batch(truths, preds):
    """The reference's score of every pair as Python floats: min(1.0, distance / (len(pred) + 1e-9)), the distance a Python int and
    len(pred) the number of symbols of the prediction."""
    lengths = preds.lengths if isinstance(preds, Packed) else [len(p) for p in preds]
    return [_score(d, n) for d, n in zip(_to_list(edit_distance_batch(truths, preds)), lengths)]


def eval(a, b):
    """editdistance.eval(a, b): the distance of one pair as a Python int."""
    return int(edit_distance_batch([a], [b])[0])


# ------------------------------------------------------------------------------------------------------- transcriptions.jsonl

def _records(records_or_path):
    if isinstance(records_or_path, (str, os.PathLike)):
        with open(records_or_path, encoding="utf-8") as f:
            return [json.loads(line) for line in f.read().splitlines() if line.strip()]
    return list(records_or_path)


def _texts(rec, renormalize):
    """truth and pred of a record.  With renormalize they are normalised again: the truth from the corpus text under meta['t'] when the
    record carries its meta, the prediction from the recogniser's NBest[0]['Lexical'] when it is there, else from the stored strings."""
    if "truth" not in rec or "pred" not in rec:
        raise B2SError("record %r has neither 'fail' nor 'truth' / 'pred'" % (rec.get("name"),))
    truth, pred = rec["truth"], rec["pred"]
    if renormalize:
        locale = rec.get("locale", "")
        meta = rec.get("meta")
        if isinstance(meta, dict) and "t" in meta:
            truth = meta["t"]
        if rec.get("NBest") and "Lexical" in rec["NBest"][0]:
            pred = rec["NBest"][0]["Lexical"]
        truth, pred = basic_normalize(truth, locale), basic_normalize(pred, locale)
    return truth, pred


def score_transcriptions(records_or_path, renormalize=False):
    """Re-score a transcriptions.jsonl (a path, or the list of its records) as eval.run_transcription reports it.  Every record without
    'fail' gets its CER recomputed from truth / pred in one batch.  Returns a dict: `n`, `n_failed`, `raw_cer` (the mean over all
    records, failed ones counting 1.0), `cers` (per record, in order) and `locales`: per locale, over the records without 'fail', `n`,
    `cer` (the mean of the per-sample scores: the eval's `cer` window), `micro_cer` (summed distances over summed prediction
    lengths; None without a predicted symbol) and the summed `sub`, `del`, `ins`, `truth_len`, `pred_len`."""
    records = _records(records_or_path)
    scored = [r for r in records if "fail" not in r]
    texts = [_texts(r, renormalize) for r in scored]
    dist, ops = [], []
    if scored:
        d, o = edit_distance_batch([t for t, _ in texts], [p for _, p in texts], return_ops=True)
        dist, ops = _to_list(d), _to_list(o)
    cers, locales, k = [], {}, 0
    for r in records:
        if "fail" in r:
            cers.append(1.0)
            continue
        truth, pred = texts[k]
        cers.append(_score(dist[k], len(pred)))
        loc = locales.setdefault(r.get("locale", ""), {"n": 0, "cer": 0.0, "dist": 0, "sub": 0, "del": 0, "ins": 0,
                                                       "truth_len": 0, "pred_len": 0})
        loc["n"] += 1
        loc["cer"] += cers[-1]                           # the window sums the values in order, then divides
        loc["dist"] += dist[k]
        for name, v in zip(OP_NAMES, ops[k]):
            loc[name] += v
        loc["truth_len"] += len(truth)
        loc["pred_len"] += len(pred)
        k += 1
    for loc in locales.values():
        loc["cer"] = loc["cer"] / loc["n"]
        d = loc.pop("dist")
        loc["micro_cer"] = d / loc["pred_len"] if loc["pred_len"] else None
    return {"n": len(records), "n_failed": len(records) - len(scored), "raw_cer": float(np.mean(cers)) if cers else None,
            "locales": locales, "cers": cers}


# ---------------------------------------------------------------------------------------------------- opt-in for the reference eval

_ORIGINAL = "_b2s_reference_editdistance"
_SHIM = types.SimpleNamespace(eval=eval)                 # what utils.transcribe sees as `editdistance`


def install(hp=None):
    """Bind the `editdistance` global of utils.transcribe (the reference's module, if imported) to this module's eval for
    hp.cer == "hip"; restore the original for "reference".  Anything else is a ValueError."""
    on = choice(hp, "cer") == "hip"
    if rebind("utils.transcribe", "editdistance", _SHIM, _ORIGINAL, on):
        logging.info("cer=hip: utils.transcribe scores with the GPU edit distance (b2s_hip.cer)" if on else
                     "cer=reference: utils.transcribe.editdistance restored")


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m b2s_hip.cer", description="Re-score a transcriptions.jsonl on the GPU.")
    ap.add_argument("path", help="transcriptions.jsonl written by eval.py")
    ap.add_argument("--renormalize", action="store_true", help="apply basic_normalize again before scoring")
    rescore.add_arguments(ap, "--json")
    a = ap.parse_args(argv)
    return rescore.finish(score_transcriptions(a.path, renormalize=a.renormalize), a.json, ("cers",), indent=1)


if __name__ == "__main__":
    sys.exit(main())
