"""with PYTHONPATH=<package>:<reference checkout> the reference's own drivers import against
this package.  The import blocks of the reference's train.py (lines 1-21) and eval.py (lines 1-22) are restated below as the
(module, names) pairs they import from the modules this package replaces or extends (their standard-library and third-party
imports left out); a fresh interpreter imports them with the package in front of a stand-in checkout that holds only the
reference's out-of-scope glue (dataloader, utils.infolog, utils.transcribe -- none of them on the hot path), and the test
checks which file every hot-path name resolved to."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import PKG

IMPORT_BLOCKS = {
    "train.py": [("utils", ["dict_send_to"]), ("hyperparams", ["hparams"]), ("transformer", ["tacotron"]), ("utils", ["infolog", "checkpoint"]),
                 ("utils.text", ["language_vec_to_id"]), ("dataloader", ["Feeder", "FeederEval"]), ("synthesize", ["eval_batch", "save_eval_results"])],
    "eval.py": [("utils", ["dict_send_to"]), ("hyperparams", ["hparams"]), ("utils.transcribe", ["transcribe", "transcribe_available"]),
                ("transformer", ["tacotron"]), ("utils", ["infolog", "checkpoint"]), ("utils.text", ["language_vec_to_id"]),
                ("dataloader", ["FeederEval"]), ("synthesize", ["eval_batch", "save_eval_results"])],
}

# the reference-only modules those blocks import: laid out as a checkout of their own, behind the package on the path
STAND_INS = {
    "dataloader.py": "class Feeder(object):\n    pass\n\n\nclass FeederEval(object):\n    pass\n",
    os.path.join("utils", "infolog.py"): "",
    os.path.join("utils", "transcribe.py"): "transcribe_available = False\n\n\ndef transcribe(*args, **kwargs):\n    raise NotImplementedError\n",
}

PROBE = textwrap.dedent('''
    import json, os, sys
    ns = {"__name__": "dropin_probe"}
    for mod, names in json.loads(sys.argv[1]):
        exec("from %s import %s" % (mod, ", ".join(names)), ns)
    import utils, synthesize, transformer.tacotron, hyperparams, utils.checkpoint, utils.text
    for name, mod in (("utils", utils), ("utils.checkpoint", utils.checkpoint), ("utils.text", utils.text), ("utils.infolog", ns["infolog"]),
                      ("synthesize", synthesize), ("transformer.tacotron", transformer.tacotron), ("hyperparams", hyperparams),
                      ("dataloader", sys.modules["dataloader"])):
        print("MOD", name, os.path.realpath(mod.__file__))
    assert ns["eval_batch"] is synthesize.eval_batch and ns["save_eval_results"] is synthesize.save_eval_results
    assert ns["dict_send_to"] is utils.dict_send_to and ns["tacotron"] is transformer.tacotron
    print("OK")
''')


def _run_probe(script, first, last, tmp_path):
    ref = tmp_path / "reference"
    for rel, text in STAND_INS.items():
        (ref / rel).parent.mkdir(parents=True, exist_ok=True)
        (ref / rel).write_text(text)
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + str(ref))
    r = subprocess.run([sys.executable, "-c", PROBE, json.dumps(IMPORT_BLOCKS[script])], env=env, cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, "import block of %s (lines %d-%d) failed:\n%s\n%s" % (script, first, last, r.stdout, r.stderr[-3000:])
    return str(ref), dict(line.split()[1:3] for line in r.stdout.splitlines() if line.startswith("MOD "))


@pytest.mark.parametrize("script,first,last", [("train.py", 1, 21), ("eval.py", 1, 22)])
def test_reference_driver_import_block(script, first, last, tmp_path):
    ref, where = _run_probe(script, first, last, tmp_path)
    pkg, ref = os.path.realpath(PKG), os.path.realpath(ref)
    for name in ("utils", "utils.checkpoint", "utils.text", "synthesize", "transformer.tacotron", "hyperparams"):
        assert where[name].startswith(pkg + os.sep), "%s resolved to %s, not to this package" % (name, where[name])
    for name in ("utils.infolog", "dataloader"):           # out-of-scope glue keeps coming from the reference checkout
        assert where[name].startswith(ref + os.sep), "%s resolved to %s" % (name, where[name])


def test_save_eval_results_writes_trimmed_mels(tmp_path):
    """<name>.npy = mel_aft[i][:generated_lengths[i]] (reference synthesize.py:79-81); a bad sample is logged, not raised."""
    import synthesize
    rng = np.random.default_rng(0)
    mel_aft = rng.standard_normal((3, 12, 80)).astype(np.float32)
    out = {"names": ["a", "b", "c"], "mel_pre": mel_aft, "mel_aft": mel_aft, "alignments": {"encdec": [rng.random((3, 2, 5, 12))]},
           "input_lengths": [5, 4, 3], "generated_lengths": [12, 7, 1]}
    synthesize.save_eval_results(**out, output_dir=str(tmp_path / "o"), n_plot_alignment=0)
    for i, n in enumerate(out["names"]):
        got = np.load(tmp_path / "o" / ("%s.npy" % n))
        assert got.shape == (out["generated_lengths"][i], 80) and np.array_equal(got, mel_aft[i][:out["generated_lengths"][i]])
    synthesize.save_eval_results(["x"], mel_aft[:1], mel_aft[:1], {"encdec": []}, [5], [None], str(tmp_path / "o"))      # logged, not raised
    assert not (tmp_path / "o" / "x.npy").exists()
