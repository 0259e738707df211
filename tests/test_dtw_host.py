"""CPU-only tests of the DTW metric's host side: the fastdtw 0.3.4 restatement (tests/dtw_ref.py) the GPU tests compare against,
the interval form of the window the kernel uses, the libb2s_metrics.so C ABI (exports, argument errors without a GPU), the
`mse_dtw` hyper-parameter and metrics.install on a stand-in utils.infolog module."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

import dtw_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "few-shot-transformer-tts_amd")


def fresh_hp(over=""):
    import hyperparams
    hp = hyperparams.hparams
    hp.override_from_dict(hyperparams.DEFAULTS)
    if over:
        hp.parse(over)
    return hp


def _monotone_paths(n, m):
    """Every path from (0, 0) to (n - 1, m - 1) with steps (1, 0), (0, 1), (1, 1)."""
    def rec(i, j):
        if (i, j) == (n - 1, m - 1):
            yield [(i, j)]
            return
        for di, dj in ((1, 0), (0, 1), (1, 1)):
            if i + di < n and j + dj < m:
                for rest in rec(i + di, j + dj):
                    yield [(i, j)] + rest
    return list(rec(0, 0))


def _random_monotone_path(rng, n, m):
    i = j = 0
    path = [(0, 0)]
    while (i, j) != (n - 1, m - 1):
        moves = [(di, dj) for di, dj in ((1, 0), (0, 1), (1, 1)) if i + di < n and j + dj < m]
        di, dj = moves[rng.integers(len(moves))]
        i, j = i + di, j + dj
        path.append((i, j))
    return path


def test_exact_dtw_equals_brute_force_enumeration():
    rng = np.random.default_rng(1)
    for n, m in itertools.product(range(1, 7), repeat=2):
        x, y = rng.standard_normal((n, 3)), rng.standard_normal((m, 3))
        cost, path = R.dtw(x, y)
        dist = np.sqrt(((x[:, None] - y[None]) ** 2).sum(-1))
        best = min(sum(dist[i, j] for i, j in p) for p in _monotone_paths(n, m))
        assert abs(cost - best) <= 1e-12 * max(1.0, best), (n, m)
        assert path[0] == (0, 0) and path[-1] == (n - 1, m - 1)
        assert abs(sum(dist[i, j] for i, j in path) - cost) <= 1e-12 * max(1.0, cost)


def test_fastdtw_with_a_radius_covering_everything_is_exact_dtw():
    rng = np.random.default_rng(2)
    for n, m in ((5, 7), (9, 4), (12, 12), (3, 11)):
        x, y = rng.standard_normal((n, 2)), rng.standard_normal((m, 2))
        assert R.fastdtw(x, y, radius=max(n, m)) == R.dtw(x, y)


def test_fastdtw_recursion_and_ties_on_a_known_case():
    # 1-D integer sequences: every distance is an integer, ties are common; the path must still start and end at the corners
    x = np.array([0, 1, 1, 2, 3, 3, 2, 0, 0, 1], float)
    y = np.array([0, 0, 1, 2, 2, 3, 2, 1, 0], float)
    cost, path = R.fastdtw(x, y, radius=1)
    assert path[0] == (0, 0) and path[-1] == (9, 8)
    assert cost == sum(abs(x[i] - y[j]) for i, j in path)
    assert cost >= R.dtw(x, y)[0]
    with pytest.raises(ValueError):
        R.fastdtw(x, y, radius=0)


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_interval_window_equals_set_form_on_random_paths(radius):
    rng = np.random.default_rng(10 + radius)
    shapes = [(1100, 40), (40, 1100), (7, 9), (9, 7), (2, 2), (3, 5)]
    for trial in range(1000):
        if trial < len(shapes):
            lx, ly = shapes[trial]
        else:
            lx, ly = (int(v) for v in rng.integers(2, 90, size=2))
        path = _random_monotone_path(rng, lx // 2, ly // 2) if min(lx, ly) >= 2 else [(0, 0)]
        lo, hi = R.window_intervals(path, lx, ly, radius)
        assert np.all(np.diff(lo) >= 0) and np.all(np.diff(hi) >= 0) and np.all(lo <= hi)
        assert R.intervals_to_window(lo, hi) == R.expand_window(path, lx, ly, radius), (lx, ly, radius, trial)


def test_interval_window_matches_fastdtw_paths():
    # the paths fastdtw itself produces (not only random ones) expand to the same window in both forms
    rng = np.random.default_rng(5)
    for n, m in ((33, 29), (41, 17), (16, 50)):
        x, y = rng.standard_normal((n // 2, 4)), rng.standard_normal((m // 2, 4))
        _, path = R.fastdtw(x, y, radius=1)
        lo, hi = R.window_intervals(path, n, m, 1)
        assert R.intervals_to_window(lo, hi) == R.expand_window(path, n, m, 1)


def test_calculate_mse_dtw_restatement_skips_unvoiced_frames_and_returns_none():
    rng = np.random.default_rng(3)
    preds = np.abs(rng.standard_normal((3, 8, 4))).astype(np.float32)
    targets = preds.copy()
    preds[1] = -1.0                                      # nothing voiced
    targets[2, :3] = -2.0                                # three unvoiced frames dropped from the target
    out = R.calculate_mse_dtw(preds, [8, 8, 8], targets, [8, 8, 6])
    assert out[0] == 0.0 and out[1] is None and isinstance(out[2], np.floating)


# ------------------------------------------------------------------------------------------------------------------- the C ABI

def test_metrics_library_exports_every_declared_symbol():
    from b2s_hip import metrics
    l = metrics.load()
    header = open(os.path.join(ROOT, "include", "b2s_metrics.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(b2s_met_[a-z0-9_]+)\s*\(", header))
    assert declared == set(metrics.EXPORTS), declared ^ set(metrics.EXPORTS)
    for name in sorted(declared):
        assert hasattr(l, name)
    assert l.b2s_met_version() >= 100
    nm = subprocess.run(["nm", "-D", "--defined-only", metrics.LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:
        exported = set(re.findall(r"\b(b2s_[a-z0-9_]+)$", nm.stdout, flags=re.M))
        assert exported == declared, exported ^ declared


def test_model_and_vocoder_libraries_carry_no_metric_symbol():
    from b2s_hip import lib, vocoder
    assert not any(n.startswith("b2s_met") for n in lib.EXPORTS + vocoder.EXPORTS)
    for path in (lib.LIB_PATH, vocoder.LIB_PATH):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
        if nm.returncode != 0:
            pytest.skip("nm is not available")
        assert "b2s_met_" not in nm.stdout, path


def test_argument_errors_come_back_as_messages_without_a_gpu():
    from b2s_hip import metrics
    l = metrics.load()

    def err():
        return l.b2s_met_last_error().decode()
    ok = l.b2s_met_dtw_ws_bytes(4, 400, 300, 100, 100, 80, 1, metrics.VOICED_ONLY)
    assert ok > 2 * 400 * 80 * 8
    assert l.b2s_met_dtw_ws_bytes(4, 400, 300, 100, 100, 80, -1, 0) >= ok          # exact mode: the full back-pointer matrix
    for dim in (0, 257, -3):
        assert l.b2s_met_dtw_ws_bytes(4, 400, 300, 100, 100, dim, 1, 0) == 0 and "dim must be in 1..256" in err()
    assert l.b2s_met_dtw_ws_bytes(4, -1, 300, 100, 100, 80, 1, 0) == 0 and "lengths must be >= 0" in err()
    assert l.b2s_met_dtw_ws_bytes(4, 400, 300, -5, 100, 80, 1, 0) == 0 and "lengths must be >= 0" in err()
    assert l.b2s_met_dtw_ws_bytes(4, 400, 300, 100, 100, 80, 0, 0) == 0 and "radius 0 is not supported" in err()
    assert l.b2s_met_dtw_ws_bytes(4, 400, 300, 100, 100, 80, -2, 0) == 0 and "radius must be >= 1, or -1" in err()
    assert l.b2s_met_dtw_ws_bytes(0, 400, 300, 100, 100, 80, 1, 0) == 0 and "B must be > 0" in err()
    assert l.b2s_met_dtw_ws_bytes(4, 400, 300, 100, 100, 80, 1, 6) == 0 and "unknown flags" in err()
    assert l.b2s_met_dtw_ws_bytes(4, 40, 300, 100, 100, 80, 1, 0) == 0 and "exceed total_x" in err()
    assert l.b2s_met_dtw_ws_bytes(1, 9000, 9000, 9000, 9000, 80, 1, 0) == 0 and "on-chip plan" in err()
    d = C.c_void_p(16)           # never dereferenced: every call below fails its checks before a launch
    args = [d, d, 400, 100, d, d, 300, 100, 4, 80, 1, 0, d, d, d, d, None, None]
    assert l.b2s_met_dtw(*args, d, ok - 1, None) != 0 and "workspace of %d bytes, %d needed" % (ok - 1, ok) in err()
    bad = list(args)
    bad[10] = 0
    assert l.b2s_met_dtw(*bad, d, ok, None) != 0 and "radius 0" in err()
    bad = list(args)
    bad[12] = None
    assert l.b2s_met_dtw(*bad, d, ok, None) != 0 and "NULL" in err()
    bad = list(args)
    bad[16] = d
    assert l.b2s_met_dtw(*bad, d, ok, None) != 0 and "path_offsets" in err()


def test_python_wrappers_refuse_bad_arguments_before_the_gpu():
    from b2s_hip import B2SError, metrics, ragged
    x = np.zeros((2, 5, 3), np.float32)
    with pytest.raises(B2SError, match="radius must be >= 1"):
        metrics.c_radius(0)
    assert metrics.c_radius(None) == -1 and metrics.c_radius(2) == 2
    with pytest.raises(B2SError, match="must be >= 0"):
        ragged.lengths([3, -1], 2, 5, "x_lengths")
    with pytest.raises(B2SError, match="3 x_lengths for a batch of 2"):
        ragged.lengths([3, 1, 2], 2, 5, "x_lengths")
    assert ragged.lengths(np.array([7, 2]), 2, 5, "x") == [5, 2]              # sliced past the end, like x[i, :n]
    packed, off = ragged.pack(ragged.as_batch(x + np.arange(5)[None, :, None], "cpu", "x"), [3, 2])
    assert packed.shape == (5, 3) and off.tolist() == [0, 3, 5] and packed[:, 0].tolist() == [0, 1, 2, 0, 1]


# ------------------------------------------------------------------------------------------------- hparam and eval.py opt-in

def test_mse_dtw_hparam_defaults_to_reference():
    import hyperparams
    hp = fresh_hp()
    assert hp.mse_dtw == "reference" and hyperparams.DEFAULTS["mse_dtw"] == "reference"
    hp.parse("mse_dtw=hip")
    assert hp.mse_dtw == "hip"
    fresh_hp()


def test_unknown_mse_dtw_is_refused():
    from b2s_hip import metrics
    hp = fresh_hp("mse_dtw=scipy")
    try:
        with pytest.raises(ValueError, match="unknown mse_dtw 'scipy'"):
            metrics.install(hp)
    finally:
        fresh_hp()


def test_install_binds_and_restores_calculate_mse_dtw_on_the_reference_module(monkeypatch):
    from b2s_hip import metrics

    def reference_impl(preds, pred_lengths, targets, target_lengths):
        return ["reference"]
    stand_in = types.ModuleType("utils.infolog")
    stand_in.calculate_mse_dtw = reference_impl
    monkeypatch.setitem(sys.modules, "utils.infolog", stand_in)
    try:
        metrics.install(fresh_hp())                                   # default: nothing is rebound
        assert stand_in.calculate_mse_dtw is reference_impl
        metrics.install(fresh_hp("mse_dtw=hip"))
        assert stand_in.calculate_mse_dtw is metrics.calculate_mse_dtw
        metrics.install(fresh_hp("mse_dtw=hip"))                      # idempotent: the original is kept, not the GPU function
        assert getattr(stand_in, metrics._ORIGINAL) is reference_impl
        metrics.install(fresh_hp())
        assert stand_in.calculate_mse_dtw is reference_impl and not hasattr(stand_in, metrics._ORIGINAL)
    finally:
        fresh_hp()


def test_install_without_the_reference_module_is_a_no_op(monkeypatch):
    from b2s_hip import metrics
    monkeypatch.delitem(sys.modules, "utils.infolog", raising=False)
    metrics.install(fresh_hp("mse_dtw=hip"))
    assert "utils.infolog" not in sys.modules
    fresh_hp()


def test_eval_batch_installs_the_metric_before_decoding(monkeypatch):
    """synthesize.eval_batch calls metrics.install(hp) first thing: with a stand-in model that fails on first use, the rebinding
    has already happened when the failure surfaces."""
    import synthesize
    from b2s_hip import metrics
    stand_in = types.ModuleType("utils.infolog")
    stand_in.calculate_mse_dtw = lambda *a: None
    monkeypatch.setitem(sys.modules, "utils.infolog", stand_in)

    class Boom(object):
        def engine(self):
            raise RuntimeError("stand-in model")
    fresh_hp("mse_dtw=hip")
    try:
        with pytest.raises(Exception):
            synthesize.eval_batch(Boom(), {"inputs": np.zeros((1, 3))})
        assert stand_in.calculate_mse_dtw is metrics.calculate_mse_dtw
    finally:
        metrics.install(fresh_hp())
    assert stand_in.calculate_mse_dtw is not metrics.calculate_mse_dtw
