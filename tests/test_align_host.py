"""CPU-only tests of the alignment-head selection's host side: the `align` hyper-parameter, the b2s_met_align_* C ABI (exports,
argument errors without a GPU), the two NumPy restatements (tests/align_ref.py) on cases whose answers follow by inspection, and
save_eval_results with and without a 'selected' result."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import align_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fresh_hp(over=""):
    import hyperparams
    hp = hyperparams.hparams
    hp.override_from_dict(hyperparams.DEFAULTS)
    if over:
        hp.parse(over)
    return hp


# ------------------------------------------------------------------------------------------------------------- hyper-parameter

def test_align_hparam_defaults_to_reference_and_parses_hip():
    import hyperparams
    from b2s_hip import alignment
    hp = fresh_hp()
    assert hp.align == "reference" and hyperparams.DEFAULTS["align"] == "reference"
    assert alignment.mode(hp) == "reference"
    hp.parse("align=hip")
    try:
        assert hp.align == "hip" and alignment.mode(hp) == "hip"
    finally:
        fresh_hp()


def test_unknown_align_is_refused_where_it_is_first_used():
    import synthesize
    from b2s_hip import alignment

    class Boom(object):
        def engine(self):
            raise RuntimeError("stand-in model: never reached")
    fresh_hp("align=matplotlib")
    try:
        with pytest.raises(ValueError, match="unknown align 'matplotlib'"):
            synthesize.eval_batch(Boom(), {"inputs": np.zeros((1, 3))})
        with pytest.raises(ValueError, match="unknown align 'matplotlib'"):
            alignment.select_alignments([np.zeros((1, 1, 2, 2), np.float32)], [2], [2])
    finally:
        fresh_hp()


# --------------------------------------------------------------------------------------------------------------------- the C ABI

NEW_SYMBOLS = ("b2s_met_align_chunk", "b2s_met_align_ws_bytes", "b2s_met_align_select")


def test_new_symbols_are_declared_exported_and_bound():
    from b2s_hip import metrics
    l = metrics.load()
    header = open(os.path.join(ROOT, "include", "b2s_metrics.h")).read()
    declared = set(re.findall(r"\b(b2s_met_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    for name in NEW_SYMBOLS:
        assert name in metrics.EXPORTS and name in metrics._PROTOS and name in declared and hasattr(l, name)
    assert len([n for n in metrics.EXPORTS if n.startswith("b2s_met_align_")]) <= 3
    assert l.b2s_met_align_chunk() > 0 and l.b2s_met_align_chunk() % 64 == 0


def test_readme_counts_the_metrics_entry_points():
    from b2s_hip import metrics
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "`libb2s_metrics.so`, %d entry points" % len(metrics.EXPORTS) in readme


def test_argument_errors_come_back_as_messages_without_a_gpu():
    from b2s_hip import metrics
    l = metrics.load()

    def err():
        return l.b2s_met_last_error().decode()
    B, L, H, S, T = 4, 2, 3, 37, 70
    ok = l.b2s_met_align_ws_bytes(B, L, H, S, T)
    assert ok >= B * L * H * T * 4 + B * L * H * 8                  # at least the per-head argmax rows and one partial per head
    for n_layers in (0, 17):
        assert l.b2s_met_align_ws_bytes(B, n_layers, H, S, T) == 0 and "n_layers must be in 1..16" in err()
    for bad, name in ((0, "B"), (-2, "B")):
        assert l.b2s_met_align_ws_bytes(bad, L, H, S, T) == 0 and "%s must be > 0" % name in err()
    for bad in (0, -1):
        assert l.b2s_met_align_ws_bytes(B, L, bad, S, T) == 0 and "H must be > 0" in err()
        assert l.b2s_met_align_ws_bytes(B, L, H, bad, T) == 0 and "S must be > 0" in err()
        assert l.b2s_met_align_ws_bytes(B, L, H, S, bad) == 0 and "T must be > 0" in err()
    d = C.c_void_p(16)               # never dereferenced: every call below fails its checks before a launch
    table = (C.c_void_p * L)(16, 16)  # the host array of layer pointers is read, what it points to is not
    tail = [d, d, d, d, None, None, None, d]

    def call(layers, n_layers, dims, ws_bytes, args=tail):
        return l.b2s_met_align_select(layers, n_layers, *dims, *args, ws_bytes, None)
    dims = [B, H, S, T]
    assert call(table, L, dims, ok - 1) != 0 and "workspace of %d bytes, %d needed" % (ok - 1, ok) in err()
    assert call(None, L, dims, ok) != 0 and "layers is NULL" in err()
    for n_layers in (0, 17):
        assert call(table, n_layers, dims, ok) != 0 and "n_layers must be in 1..16" in err()
    for k, name in enumerate("BHST"):
        for v in (0, -3):
            bad = list(dims)
            bad[k] = v
            assert call(table, L, bad, ok) != 0 and "%s must be > 0" % name in err()
    assert call((C.c_void_p * L)(16, None), L, dims, ok) != 0 and "layers[1] is NULL" in err()
    assert call(table, L, dims, ok, [None] + tail[1:]) != 0 and "enc_len" in err()
    assert call(table, L, dims, ok, tail[:3] + [None] + tail[4:]) != 0 and "best_out" in err()
    assert call(table, L, dims, ok, tail[:7] + [None]) != 0 and "ws is NULL" in err()


# ------------------------------------------------------------------------------------------------------------ the restatements

def _both(layers, enc, dec):
    """Restatement (a), and restatement (b)'s choice per utterance as l * H + h."""
    a = R.select(layers, enc, dec)
    H = layers[0].shape[1]
    b = []
    for i in range(layers[0].shape[0]):
        k, h, crop = R.plot_attn_choice([l[i].transpose(0, 2, 1) for l in layers], enc[i], dec[i])
        b.append(k * H + h if k >= 0 else -1)
        if k >= 0 and a["best"][i] >= 0:
            e, d = enc[i] or None, dec[i] or None
            assert np.array_equal(crop, a["maps"][i].T[:d, :e])
    return a, b


def _uniform(B, H, S, T):
    return np.full((B, H, S, T), 1.0 / S, np.float32)


def test_one_hot_diagonal_head_among_uniform_heads():
    S = T = 8
    layers = [_uniform(1, 3, S, T), _uniform(1, 3, S, T)]
    layers[1][0, 1] = np.eye(S, dtype=np.float32)
    a, b = _both(layers, [S], [T])
    assert a["best"].tolist() == [4] and b == [4]
    assert a["scores"][0, 1, 1] == T and np.allclose(a["scores"][0, 0], T / S)
    assert a["paths"][0].tolist() == list(range(T))
    assert a["stats"][0].tolist() == [0, 1, S, S - 1]
    assert np.array_equal(a["maps"][0], np.eye(S, dtype=np.float32))


def test_lengths_crop_the_score_and_the_path():
    S, T = 8, 10
    layers = [_uniform(1, 2, S, T)]
    layers[0][0, 1, 6, :] = 0.9                         # a bright row past enc_len must not count
    layers[0][0, 0, 2, :4] = 0.5
    a, b = _both(layers, [5], [4])
    assert a["best"].tolist() == [0] and b == [0]
    assert a["scores"][0, 0, 0] == 2.0 and a["scores"][0, 0, 1] == pytest.approx(0.5)
    assert a["paths"][0].tolist() == [2, 2, 2, 2] + [-1] * 6
    assert a["stats"][0].tolist() == [0, 0, 1, 2]


def test_two_identical_best_heads_the_earlier_wins():
    S = T = 6
    layers = [_uniform(1, 2, S, T), _uniform(1, 2, S, T)]
    layers[0][0, 1] = np.eye(S, dtype=np.float32)
    layers[1][0, 0] = np.eye(S, dtype=np.float32)
    a, b = _both(layers, [S], [T])
    assert a["scores"][0, 0, 1] == a["scores"][0, 1, 0]
    assert a["best"].tolist() == [1] and b == [1]


def test_all_zero_input_and_zero_lengths_give_no_choice():
    layers = [np.zeros((3, 2, 4, 5), np.float32)]
    layers[0][1:] = 0.25
    a, b = _both(layers, [4, 4, 0], [5, 0, 5])
    assert a["best"].tolist() == [-1, -1, -1]
    assert b[0] == -1                                   # (b) with a length of 0 does not crop: only the all-zero case is comparable
    assert not a["maps"].any() and (a["paths"] == -1).all() and not a["stats"].any() and not a["scores"].any()


def test_path_with_a_known_backward_step_and_jump():
    S, T = 9, 6
    path = [0, 1, 5, 3, 3, 8]                           # one backward step (5 -> 3), largest forward jump 5 (3 -> 8), 5 positions
    head = np.full((S, T), 0.01, np.float32)
    head[path, np.arange(T)] = 0.8
    head[4, 3] = 0.8                                    # a tie at frame 3: the first maximum (row 3) is the path
    layers = [np.stack([_uniform(1, 1, S, T)[0, 0], head])[None]]
    a, b = _both(layers, [S], [T])
    assert a["best"].tolist() == [1] and b == [1]
    assert a["paths"][0].tolist() == path
    assert a["stats"][0].tolist() == [1, 5, 5, 8]


def test_generator_gaps_hold_for_the_gpu_cases():
    """The GPU test compares with the reference's fp32 loop only where the fp64 gap between the best two scores is >= 1e-3 * dec_len;
    its generator and seeds are checked here, where no GPU is needed."""
    from b2s_hip import alignment
    for name, (B, L, H, S, T, enc, dec) in R.gpu_cases(alignment.chunk()).items():     # the library loads without a GPU
        layers = R.make_case(R.SEED, B, L, H, S, T, enc, dec)
        a, b = _both(layers, enc, dec)
        for i in range(B):
            if dec[i] > 0:
                assert R.best_gap(a["scores"][i]) >= 1e-3 * dec[i], (name, i)
                assert b[i] == a["best"][i], (name, i)


# --------------------------------------------------------------------------------------------------------- save_eval_results

def _selected_results():
    S, T = 7, 9
    maps = np.zeros((3, 1, S, T), np.float32)
    maps[0, 0, np.minimum(np.arange(T), S - 1), np.arange(T)] = 1.0
    maps[1, 0, 0, :] = 0.5
    scores = np.zeros((3, 2, 2))
    scores[0, 1, 0], scores[1, 0, 1] = 9.0, 2.0
    selected = {"layer": np.array([1, 0, -1], np.int32), "head": np.array([0, 1, -1], np.int32), "scores": scores,
                "focus": np.array([1.0, 0.5, 0.0]), "stats": np.array([[0, 1, 7, 6], [0, 0, 1, 0], [0, 0, 0, 0]], np.int32)}
    mel = np.random.default_rng(0).standard_normal((3, T, 4)).astype(np.float32)
    return dict(names=["a", "b", "c"], mel_pre=mel, mel_aft=mel, alignments={"self": [], "encdec": [maps], "selected": selected},
                input_lengths=[7, 5, 3], generated_lengths=[9, 4, 0])


def test_save_eval_results_writes_the_selected_alignment(tmp_path, caplog):
    import synthesize
    fresh_hp()
    res = _selected_results()
    synthesize.save_eval_results(**res, output_dir=str(tmp_path))
    for name in "abc":
        assert (tmp_path / ("%s.npy" % name)).exists()
    got = json.load(open(tmp_path / "a_align.json"))
    assert got == {"layer": 1, "head": 0, "score": 9.0, "focus": 1.0, "backward_steps": 0, "max_jump": 1, "positions_visited": 7,
                   "last_position": 6}
    assert all(type(v) in (int, float) for v in got.values())
    assert json.load(open(tmp_path / "b_align.json"))["head"] == 1
    assert not (tmp_path / "c_align.json").exists() and not (tmp_path / "c_align.png").exists()      # no choice: logged and skipped
    assert "Fail to produce eval output: c" in caplog.text
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return
    assert (tmp_path / "a_align.png").stat().st_size > 0 and (tmp_path / "b_align.png").exists()


def test_save_eval_results_honours_n_plot_alignment(tmp_path):
    import synthesize
    fresh_hp()
    synthesize.save_eval_results(**_selected_results(), output_dir=str(tmp_path), n_plot_alignment=1)
    assert (tmp_path / "a_align.json").exists() and not (tmp_path / "b_align.json").exists()
    assert (tmp_path / "b.npy").exists()


def test_save_eval_results_without_selected_is_unchanged(tmp_path):
    """A reference-style `alignments` (every layer, no 'selected'): without the reference's utils.infolog on the path only the .npy
    files are written, as before."""
    import synthesize
    fresh_hp()
    res = _selected_results()
    res["alignments"] = {"self": [], "encdec": [np.zeros((3, 2, 7, 9), np.float32)] * 2}
    synthesize.save_eval_results(**res, output_dir=str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["a.npy", "b.npy", "c.npy"]


def test_alignment_figures_stay_out_of_a_pyplot_users_way(tmp_path, monkeypatch):
    """With a reference checkout on the path, plot_mel draws through pyplot under utils.infolog.lock in the same worker threads.
    pyplot's current figure is process-wide, so the alignment figure must not go through pyplot outside that lock: here every
    pyplot call made without the stand-in's lock held is recorded, and every picture must come out whole."""
    import sys
    import threading
    import types
    matplotlib = pytest.importorskip("matplotlib")
    matplotlib.use("Agg")
    from matplotlib import pyplot as plt
    import synthesize
    import utils

    stub = types.ModuleType("utils.infolog")
    stub.lock = threading.Lock()
    owner, outside, mel_sizes = [None], [], []

    def guarded(fn):
        def call(*a, **kw):
            if owner[0] != threading.get_ident():
                outside.append(fn.__name__)
            return fn(*a, **kw)
        return call
    for fn in ("figure", "pcolor", "title", "savefig", "close", "gcf", "gca"):
        monkeypatch.setattr(plt, fn, guarded(getattr(plt, fn)))

    def plot_mel(path, mel, title=''):
        with stub.lock:
            owner[0] = threading.get_ident()
            try:
                assert plt.get_fignums() == []                    # nobody else's figure is current
                fig = plt.figure(figsize=(6, 2))
                plt.pcolor(np.asarray(mel).T)
                plt.title(title)
                assert plt.gcf() is fig
                plt.savefig(path)
                mel_sizes.append(tuple(fig.get_size_inches()))
                plt.close()
            finally:
                owner[0] = None

    def plot_attn(*a, **kw):
        raise AssertionError("with 'selected' the reference's plot_attn is not called")
    stub.plot_mel, stub.plot_attn = plot_mel, plot_attn
    monkeypatch.setitem(sys.modules, "utils.infolog", stub)
    monkeypatch.setattr(utils, "infolog", stub, raising=False)

    fresh_hp()
    res = _selected_results()
    n = 12                                                        # more samples than workers, so the two kinds of plot interleave
    res["names"] = ["s%02d" % i for i in range(n)]
    for k in ("mel_pre", "mel_aft"):
        res[k] = np.concatenate([res[k][:2]] * (n // 2))
    res["alignments"]["encdec"] = [np.concatenate([res["alignments"]["encdec"][0][:2]] * (n // 2))]
    res["alignments"]["selected"] = {k: np.concatenate([v[:2]] * (n // 2)) for k, v in res["alignments"]["selected"].items()}
    res["input_lengths"], res["generated_lengths"] = [7, 5] * (n // 2), [9, 4] * (n // 2)
    synthesize.save_eval_results(**res, output_dir=str(tmp_path))
    assert outside == [] and plt.get_fignums() == []
    assert mel_sizes == [(6.0, 2.0)] * n
    from matplotlib import image
    dpi = matplotlib.rcParams["figure.dpi"]
    for name in res["names"]:
        assert image.imread(str(tmp_path / ("%s_mel.png" % name))).shape[:2] == (int(2 * dpi), int(6 * dpi))
        assert image.imread(str(tmp_path / ("%s_align.png" % name))).shape[:2] == (int(7 * dpi), int(14 * dpi))
        assert (tmp_path / ("%s_align.json" % name)).exists()
