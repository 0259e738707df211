"""CPU-only tests of what the re-scoring tools share (b2s_hip.rescore): the walker over EVAL_DIR and mels.zip with a stub callback,
the padder, the language map, the summariser against means written out here, and the command-line pieces.  No library is loaded."""
import argparse
import json
import types
import zipfile

import numpy as np
import pytest

NAMES = "abcdefg"
FRAMES = {"a": 2, "b": 5, "c": 3, "d": 4, "e": 2, "f": 4, "g": 5}


def mel(name, bins=3, offset=0.0):
    """[frames, bins] float64 without a zero in it, its own for every name and side."""
    return 1.0 + offset + NAMES.index(name) + np.arange(FRAMES[name] * bins, dtype=np.float64).reshape(FRAMES[name], bins) / 100.0


@pytest.fixture
def finished_eval(tmp_path):
    """EVAL_DIR with a..g .npy (2..5 frames x 3 bins) and a notes.txt, and a mels.zip that holds every name but d."""
    ev = tmp_path / "eval"
    ev.mkdir()
    for n in NAMES:
        np.save(ev / (n + ".npy"), mel(n))
    (ev / "notes.txt").write_text("not a mel")
    with zipfile.ZipFile(tmp_path / "mels.zip", "w") as z:
        for n in NAMES.replace("d", ""):
            with z.open(n + ".npy", "w") as f:
                np.save(f, mel(n, offset=0.5)[:-1])
    return str(ev), str(tmp_path / "mels.zip")


def collect(ev, zp, batch):
    from b2s_hip import rescore
    calls = []
    without = rescore.walk(ev, zp, batch, lambda *args: calls.append(args))
    return calls, without


# --------------------------------------------------------------------------------------------------------------------- the walker

def test_walk_batches_the_pairs_that_have_a_target(finished_eval):
    calls, without = collect(*finished_eval, batch=3)
    assert [c[0] for c in calls] == [["a", "b", "c"], ["e", "f", "g"]] and without == ["d"]
    for batch, n_calls in ((1, 6), (100, 1), (0, 6), (-3, 6)):
        calls, without = collect(*finished_eval, batch=batch)
        assert len(calls) == n_calls and without == ["d"]
        assert [n for c in calls for n in c[0]] == list("abcefg")
    assert [c[0] for c in collect(*finished_eval, batch=4)[0]] == [["a", "b", "c", "e"], ["f", "g"]]     # d does not count


def test_walk_hands_over_padded_float32_arrays_with_their_lengths(finished_eval):
    for part, preds, pl, targets, tl in collect(*finished_eval, batch=3)[0]:
        assert pl == [FRAMES[n] for n in part] and tl == [FRAMES[n] - 1 for n in part]
        for arr, lengths, offset, cut in ((preds, pl, 0.0, None), (targets, tl, 0.5, -1)):
            assert arr.dtype == np.float32 and arr.shape == (len(part), max(lengths), 3)
            for i, n in enumerate(part):
                assert np.array_equal(arr[i, :lengths[i]], mel(n, offset=offset)[:cut].astype(np.float32))
                assert not arr[i, lengths[i]:].any()


def test_walk_refuses_a_generated_file_of_another_shape(finished_eval):
    from b2s_hip import B2SError, rescore
    ev, zp = finished_eval
    np.save(ev + "/f.npy", mel("f", bins=4))
    with pytest.raises(B2SError) as e:
        rescore.walk(ev, zp, 3, lambda *args: None)
    assert str(e.value) == "generated f.npy has shape (4, 4), expected [frames, 3]"
    with pytest.raises(B2SError) as e:
        rescore.pad([np.zeros((2, 3)), np.zeros(3)], ["x", "y"], 3, "target")
    assert str(e.value) == "target y.npy has shape (3,), expected [frames, 3]"
    out, n = rescore.pad([np.zeros((0, 3))], ["x"], 3, "target")
    assert out.shape == (1, 1, 3) and n == [0]                      # an utterance without frames still has a row to point at


def test_walk_closes_the_zip_when_the_callback_raises_and_when_it_does_not(finished_eval, monkeypatch):
    from b2s_hip import corpus, rescore
    ev, zp = finished_eval
    opened, real = [], corpus.MelZip

    class Recording(real):
        def __init__(self, path):
            real.__init__(self, path)
            self.closed = 0
            opened.append(self)

        def close(self):
            self.closed += 1
            real.close(self)
    monkeypatch.setattr(corpus, "MelZip", Recording)

    def fail(*args):
        raise RuntimeError("the scorer gave up")
    with pytest.raises(RuntimeError, match="^the scorer gave up$"):
        rescore.walk(ev, zp, 3, fail)
    rescore.walk(ev, zp, 3, lambda *args: None)
    assert [(z.path, z.closed) for z in opened] == [(zp, 1), (zp, 1)]


def test_walk_of_an_empty_directory_makes_no_call(finished_eval, tmp_path):
    empty = tmp_path / "empty"
    empty.mkdir()
    (empty / "notes.txt").write_text("nothing generated")
    assert collect(str(empty), finished_eval[1], 3) == ([], [])


def test_language_map(tmp_path):
    from b2s_hip import rescore
    hp = types.SimpleNamespace(data_format="nlti")
    meta = tmp_path / "metadata.eval.txt"
    meta.write_text("a.npy|2|text a|en-us\nb|5|text b|de-de\n", encoding="utf-8")
    assert rescore.languages(str(meta), hp) == {"a": "en-us", "b": "de-de"}
    assert rescore.languages(None, hp) == {} and rescore.languages(str(tmp_path / "nowhere.txt"), hp) == {}


# ----------------------------------------------------------------------------------------------------------------- the summariser

def test_summary_means_overall_and_per_language():
    from b2s_hip import rescore
    nan = float("nan")
    records = [{"name": "a", "language": "en-us", "x": 1.0, "y": 10.0, "z": None},
               {"name": "b", "language": "de-de", "x": 2.0, "y": nan, "z": None},
               {"name": "c", "language": "en-us", "x": 4.0, "y": 20.0, "z": nan},
               {"name": "d", "language": None, "x": None, "y": 40.0, "z": None},
               {"name": "e", "language": "en-us", "x": 100.0, "y": 100.0, "z": None}]                  # not among the scored
    res = rescore.summary({"metric": "test", "radius": 1}, records, records[:4], ["q"], ("x", "y", "z"))
    assert list(res) == ["metric", "radius", "n_scored", "n_empty", "n_without_target", "x", "y", "z", "languages", "without_target",
                         "records"]
    assert (res["metric"], res["radius"], res["n_scored"], res["n_empty"], res["n_without_target"]) == ("test", 1, 4, 1, 1)
    assert res["x"] == 7.0 / 3.0 and res["y"] == 70.0 / 3.0 and res["z"] is None
    assert res["languages"] == {"None": {"n": 1, "x": None, "y": 40.0, "z": None},
                                "de-de": {"n": 1, "x": 2.0, "y": None, "z": None},
                                "en-us": {"n": 2, "x": 2.5, "y": 15.0, "z": None}}
    assert list(res["languages"]) == ["None", "de-de", "en-us"] and list(res["languages"]["en-us"]) == ["n", "x", "y", "z"]
    assert res["without_target"] == ["q"] and res["records"] is records
    none = rescore.summary({}, [], [], [], ("x",))
    assert none == {"n_scored": 0, "n_empty": 0, "n_without_target": 0, "x": None, "languages": {}, "without_target": [],
                    "records": []}


# ---------------------------------------------------------------------------------------------------------- the command-line pieces

def tool(argv):
    """A main() as the tools write theirs: the shared arguments, then the shared checks in the tools' order."""
    from b2s_hip import rescore

    @rescore.cli
    def main(argv=None):
        ap = argparse.ArgumentParser(prog="tool")
        rescore.add_arguments(ap, "eval_dir", "--data-dir", "--zipfilepath", "--eval-meta", "--radius", "--batch", "--json")
        a = ap.parse_args(argv)
        zipfilepath, eval_meta = rescore.inputs(a)
        radius = rescore.radius(a.radius)
        rescore.batch(a.batch)
        rescore.found("EVAL_DIR", a.eval_dir, isdir=True)
        rescore.found("mels.zip", zipfilepath)
        res = {"radius": radius, "batch": a.batch, "zip": zipfilepath, "meta": eval_meta, "records": [1, 2], "without_target": ["d"]}
        return rescore.finish(res, a.json, ("records", "without_target"))
    return main(argv)


def test_radius_parses_or_is_a_usage_error(finished_eval, capsys):
    from b2s_hip import rescore
    assert rescore.radius("1") == 1 and rescore.radius("7") == 7 and rescore.radius("exact") is None
    ev, zp = finished_eval
    for bad in ("0", "-2", "abc", "1.5"):
        with pytest.raises(rescore.UsageError):
            rescore.radius(bad)
        assert tool([ev, "--data-dir", ev, "--zipfilepath", zp, "--radius=" + bad]) == 2
        captured = capsys.readouterr()
        assert captured.err == "--radius must be an integer >= 1 or 'exact' (got %r)\n" % bad and captured.out == ""


def test_batch_and_missing_inputs_are_usage_errors(finished_eval, tmp_path, capsys):
    ev, zp = finished_eval
    assert tool([ev, "--data-dir", ev, "--zipfilepath", zp, "--batch", "0"]) == 2
    assert capsys.readouterr().err == "--batch must be >= 1 (got 0)\n"
    nowhere = str(tmp_path / "nowhere")
    assert tool([nowhere, "--data-dir", str(tmp_path)]) == 2
    assert capsys.readouterr().err == "EVAL_DIR not found: %s\n" % nowhere
    assert tool([zp, "--data-dir", str(tmp_path)]) == 2                                          # a file is not a directory
    assert capsys.readouterr().err == "EVAL_DIR not found: %s\n" % zp
    assert tool([ev, "--data-dir", ev]) == 2                                                     # the default: DATA_DIR/mels.zip
    assert capsys.readouterr().err == "mels.zip not found: %s/mels.zip\n" % ev
    assert tool([ev, "--data-dir", str(tmp_path), "--zipfilepath", ev]) == 2                     # a directory is not a file
    assert capsys.readouterr().err == "mels.zip not found: %s\n" % ev
    from b2s_hip import rescore
    for what in ("checkpoint", "metadata"):
        with pytest.raises(rescore.UsageError, match="^%s not found: %s$" % (what, nowhere)):
            rescore.found(what, nowhere)
    with pytest.raises(SystemExit):                                                              # argparse's own refusals stay argparse's
        tool([])
    capsys.readouterr()


def test_finish_writes_the_file_and_hides_the_bulky_keys_on_stdout(finished_eval, tmp_path, capsys):
    from b2s_hip import rescore
    ev, zp = finished_eval
    out = tmp_path / "res.json"
    assert tool([ev, "--data-dir", str(tmp_path), "--radius", "exact", "--json", str(out)]) == 0
    want = {"radius": None, "batch": 64, "zip": zp, "meta": str(tmp_path / "metadata.eval.txt"), "records": [1, 2],
            "without_target": ["d"]}
    captured = capsys.readouterr()
    shown = {k: v for k, v in want.items() if k not in ("records", "without_target")}
    assert captured.out == json.dumps(shown) + "\n" and captured.err == ""
    assert out.read_text(encoding="utf-8") == json.dumps(want, ensure_ascii=False, indent=1)
    assert tool([ev, "--data-dir", str(tmp_path), "--eval-meta", "m.txt", "--radius", "3", "--batch", "5"]) == 0
    assert json.loads(capsys.readouterr().out) == {"radius": 3, "batch": 5, "zip": zp, "meta": "m.txt"}
    assert rescore.finish({"name": "é", "cers": [1.0]}, None, ("cers",), indent=1) == 0     # cer's tail: indented, not escaped
    assert capsys.readouterr().out == '{\n "name": "é"\n}\n'
