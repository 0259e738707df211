"""What a command-line tool that re-scores a finished eval shares with the next one, and nothing specific to one metric: the padder,
the language map, the walker over EVAL_DIR and mels.zip (walk), the summariser (summary) and the command-line pieces (cli,
add_arguments, inputs, radius, batch, found, finish).  b2s_hip.mcd and b2s_hip.f0 supply the scoring callback and the names of their
scores; b2s_hip.durations and b2s_hip.cer use the command-line pieces.
"""
import functools
import json
import math
import os
import sys

import numpy as np

from .cbind import B2SError, default_hp


def pad(mels, names, n_mels, what):
    """Ragged list of [T, n_mels] arrays -> padded fp32 [B, max T, n_mels] and the lengths; a file of another shape is a B2SError
    that names it."""
    for m, name in zip(mels, names):
        if m.ndim != 2 or int(m.shape[1]) != n_mels:
            raise B2SError("%s %s.npy has shape %s, expected [frames, %d]" % (what, name, tuple(m.shape), n_mels))
    n = [int(m.shape[0]) for m in mels]
    out = np.zeros((len(mels), max(max(n), 1), n_mels), np.float32)
    for i, m in enumerate(mels):
        out[i, :n[i]] = m
    return out, n


def languages(eval_meta, hp=None):
    """{name: language} of a metadata file (a trailing .npy of the name dropped); empty for None or a file that is not there."""
    from . import corpus
    lang = {}
    if eval_meta and os.path.exists(eval_meta):
        for row in corpus.read_metadata(eval_meta, default_hp(hp).data_format):
            lang[row["n"][:-4] if row["n"].endswith(".npy") else row["n"]] = row["i"]
    return lang


def walk(eval_dir, zipfilepath, batch, score):
    """Every `<name>.npy` of eval_dir, in sorted order, against member `<name>.npy` of the mels.zip: score(names, preds, pred_lengths,
    targets, target_lengths) is called per `batch` pairs that have a target (and for what remains), with both sides padded by pad
    to the mel bins of the batch's first target, so only one batch of mels is in memory at a time.  Returns the names that are
    generated but not a member of the zip; they are not scored."""
    from . import corpus
    batch = max(1, int(batch))
    names = sorted(f[:-4] for f in os.listdir(eval_dir) if f.endswith(".npy"))
    mels = corpus.MelZip(zipfilepath)
    no_target = []

    def flush(part, truth):
        n_mels = int(truth[0].shape[-1])
        targets, tl = pad(truth, part, n_mels, "target")
        preds, pl = pad([np.load(os.path.join(eval_dir, n + ".npy")).astype(np.float32) for n in part], part, n_mels, "generated")
        score(part, preds, pl, targets, tl)
    try:
        part, truth = [], []
        for n in names:
            try:
                truth.append(mels.load(n + ".npy").astype(np.float32))
            except KeyError:
                no_target.append(n)
                continue
            part.append(n)
            if len(part) == batch:
                flush(part, truth)
                part, truth = [], []
        if part:
            flush(part, truth)
    finally:
        mels.close()
    return no_target


def means(records, keys):
    """{"n": len(records), key: mean over the records, ...}; a None or NaN is left out of its key's mean, no value at all gives None."""
    out = {"n": len(records)}
    for k in keys:
        v = [r[k] for r in records if r[k] is not None and not math.isnan(r[k])]
        out[k] = float(np.mean(v)) if v else None
    return out


def summary(head, records, scored, without_target, keys):
    """The result dict of a re-scoring run: `head` (metric, radius, ...), the counts, the overall means of `keys` over the `scored`
    records, the same per str(language) with its n, the names without a target and all the records."""
    by_language = {}
    for r in scored:
        by_language.setdefault(str(r["language"]), []).append(r)
    res = dict(head, n_scored=len(scored), n_empty=len(records) - len(scored), n_without_target=len(without_target))
    res.update({k: v for k, v in means(scored, keys).items() if k != "n"})
    res.update(languages={k: means(v, keys) for k, v in sorted(by_language.items())}, without_target=without_target, records=records)
    return res


# -------------------------------------------------------------------------------------------------------------------- command line

class UsageError(Exception):
    pass


def cli(main):
    """Decorator of a main(argv=None): a UsageError raised inside becomes its one line on stderr and the return code 2."""
    @functools.wraps(main)
    def run(argv=None):
        try:
            return main(argv)
        except UsageError as e:
            print(e, file=sys.stderr)
            return 2
    return run


_ARGUMENTS = {
    "eval_dir": {"help": "directory of generated mels, <name>.npy as save_eval_results writes them"},
    "--data-dir": {"required": True, "help": "directory of mels.zip and metadata.eval.txt"},
    "--zipfilepath": {"help": "the ground-truth mels (default: DATA_DIR/mels.zip)"},
    "--eval-meta": {"help": "metadata with the languages (default: DATA_DIR/metadata.eval.txt)"},
    "--radius": {"default": "1", "help": "fastdtw radius >= 1, or 'exact' for the full dtw"},
    "--batch": {"type": int, "default": 64, "help": "pairs per GPU call"},
    "--json": {"metavar": "OUT", "help": "also write the summary, with the per-record scores, to OUT"},
}


def add_arguments(ap, *names):
    """The shared arguments `names` on an argparse parser, in that order."""
    for name in names:
        ap.add_argument(name, **_ARGUMENTS[name])


def inputs(a):
    """(zipfilepath, eval_meta) of parsed arguments, DATA_DIR's files unless given."""
    return a.zipfilepath or os.path.join(a.data_dir, "mels.zip"), a.eval_meta or os.path.join(a.data_dir, "metadata.eval.txt")


def radius(text):
    """--radius as the scoring calls take it: None for 'exact', else the integer >= 1."""
    try:
        r = None if text == "exact" else int(text)
    except ValueError:
        r = 0
    if r is not None and r < 1:
        raise UsageError("--radius must be an integer >= 1 or 'exact' (got %r)" % text)
    return r


def batch(n):
    if n < 1:
        raise UsageError("--batch must be >= 1 (got %d)" % n)
    return n


def found(what, path, isdir=False):
    if not (os.path.isdir if isdir else os.path.isfile)(path):
        raise UsageError("%s not found: %s" % (what, path))


def finish(res, json_path, hidden, indent=None):
    """The tail of a tool: the whole result to json_path if given, and without its bulky `hidden` keys on stdout."""
    if json_path:
        with open(json_path, "w", encoding="utf-8") as f:
            json.dump(res, f, ensure_ascii=False, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k not in hidden}, ensure_ascii=False, indent=indent))
    return 0
