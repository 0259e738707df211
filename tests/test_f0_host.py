"""CPU-only tests of the F0 feature's host side: the C ABI of libb2s_f0.so (declared, exported, bound, kept apart from the other
libraries; every host-side refusal without a GPU), the command line's usage errors, and the NumPy restatement (tests/f0_ref.py) on
properties known in closed form."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import f0_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = ["b2s_f0_last_error", "b2s_f0_quantize", "b2s_f0_score", "b2s_f0_version", "b2s_f0_yin"]


# --------------------------------------------------------------------------------------------------------------------- the C ABI

def test_header_exports_and_prototypes_are_the_same_five_names():
    from b2s_hip import f0
    l = f0.load()
    header = open(os.path.join(ROOT, "include", "b2s_f0.h")).read()
    declared = sorted(set(re.findall(r"\b(b2s_f0_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert declared == f0.EXPORTS == sorted(f0._PROTOS) == ENTRY_POINTS
    for name in ENTRY_POINTS:
        assert hasattr(l, name)
    assert l.b2s_f0_version() >= 100


def test_the_other_libraries_do_not_grow():
    from b2s_hip import lib, mcd, metrics, vocoder
    for mod in (lib, vocoder, metrics, mcd):
        assert not [n for n in mod.EXPORTS if n.startswith("b2s_f0")]
    assert (len(vocoder.EXPORTS), len(metrics.EXPORTS), len(mcd.EXPORTS)) == (13, 9, 5)


def test_readme_carries_the_entry_point_count():
    assert "`libb2s_f0.so`, %d entry points" % len(ENTRY_POINTS) in open(os.path.join(ROOT, "README.md")).read()


def test_importing_the_module_leaves_the_hyperparameters_alone():
    import hyperparams
    before = dict(hyperparams.DEFAULTS)
    from b2s_hip import f0  # noqa: F401
    assert hyperparams.DEFAULTS == before
    assert not [k for k in hyperparams.DEFAULTS if k.startswith("f0") or k.startswith("yin")]


def test_host_side_refusals_come_back_as_messages_without_a_gpu():
    from b2s_hip import f0
    l = f0.load()

    def err():
        return l.b2s_f0_last_error().decode()
    d = C.c_void_p(16)                   # never dereferenced: every call below fails its checks before a launch

    def quant(wav=d, lengths=d, B=2, Lmax=100, pcm=d, status=d):
        return l.b2s_f0_quantize(wav, lengths, B, Lmax, pcm, None, status, None)
    for bad in (0, -1):
        assert quant(B=bad) != 0 and "B must be > 0 (got %d)" % bad in err()
    assert quant(Lmax=-1) != 0 and "Lmax must be >= 0 (got -1)" in err()
    for name in ("lengths", "status"):
        assert quant(**{name: None}) != 0 and "lengths or status is NULL" in err()
    for name in ("wav", "pcm"):
        assert quant(**{name: None}) != 0 and "wav or pcm is NULL" in err()

    good = dict(pcm=d, lengths=d, off=d, total=10, B=2, Lmax=100, win=800, hop=200, tau_min=32, tau_max=266, threshold=0.1,
                min_energy=0, sr=16000.0, f0=d, tau=d, status=d)

    def yin(**over):
        v = dict(good, **over)
        return l.b2s_f0_yin(v["pcm"], v["lengths"], v["off"], v["total"], v["B"], v["Lmax"], v["win"], v["hop"], v["tau_min"],
                            v["tau_max"], v["threshold"], v["min_energy"], v["sr"], v["f0"], v["tau"], None, None, v["status"], None)
    for bad in (0, -5):
        assert yin(B=bad) != 0 and "B must be > 0 (got %d)" % bad in err()
    assert yin(Lmax=-1) != 0 and "Lmax must be >= 0" in err()
    assert yin(total=-1) != 0 and "total_frames must be >= 0 (got -1)" in err()
    for bad in (1, 0, -800, 2049):
        assert yin(win=bad) != 0 and "win must be in 2..2048 (got %d)" % bad in err()
    for bad in (0, -1):
        assert yin(hop=bad) != 0 and "hop must be >= 1 (got %d)" % bad in err()
    for lo, hi in ((1, 266), (0, 266), (266, 266), (300, 266), (32, 513), (-3, 10)):
        assert yin(tau_min=lo, tau_max=hi) != 0 and "need 2 <= tau_min < tau_max <= 512 (got %d and %d)" % (lo, hi) in err()
    for bad in (0.0, -0.1, float("nan")):
        assert yin(threshold=bad) != 0 and "threshold must be > 0" in err()
    assert yin(min_energy=-1) != 0 and "min_energy must be >= 0 (got -1)" in err()
    for bad in (0.0, -16000.0, float("nan")):
        assert yin(sr=bad) != 0 and "sr must be > 0" in err()
    for name in ("lengths", "off", "status"):
        assert yin(**{name: None}) != 0 and "lengths, frame_offsets or status is NULL" in err()
    assert yin(pcm=None) != 0 and "pcm is NULL" in err()
    for name in ("f0", "tau"):
        assert yin(**{name: None}) != 0 and "f0_out or tau_out is NULL" in err()
    assert yin(B=1 << 30, Lmax=1 << 30, hop=1) != 0 and "split the batch" in err()

    sgood = dict(f0x=d, taux=d, fxo=d, tfx=10, f0y=d, tauy=d, fyo=d, tfy=10, kx=d, kxo=d, tkx=8, ky=d, kyo=d, tky=8, B=2, path=d,
                 po=d, tp=20, plen=d, dstat=d, gross=0.2, scores=d, counts=d, status=d)

    def score(**over):
        v = dict(sgood, **over)
        return l.b2s_f0_score(v["f0x"], v["taux"], v["fxo"], v["tfx"], v["f0y"], v["tauy"], v["fyo"], v["tfy"], v["kx"], v["kxo"],
                              v["tkx"], v["ky"], v["kyo"], v["tky"], v["B"], v["path"], v["po"], v["tp"], v["plen"], v["dstat"],
                              v["gross"], v["scores"], v["counts"], v["status"], None)
    for bad in (0, -3):
        assert score(B=bad) != 0 and "B must be > 0 (got %d)" % bad in err()
    for name in ("tfx", "tfy", "tkx", "tky", "tp"):
        assert score(**{name: -1}) != 0 and "totals must be >= 0" in err()
    for bad in (-0.1, float("nan")):
        assert score(gross=bad) != 0 and "gross_ratio must be >= 0" in err()
    for name in ("fxo", "fyo", "kxo", "kyo", "po", "plen", "dstat"):
        assert score(**{name: None}) != 0 and "is NULL" in err() and "path_offsets" in err()
    for name in ("f0x", "taux", "f0y", "tauy"):
        assert score(**{name: None}) != 0 and "an F0 or tau buffer is NULL" in err()
    for name in ("kx", "ky", "path"):
        assert score(**{name: None}) != 0 and "kept_x, kept_y or path is NULL" in err()
    for name in ("scores", "counts", "status"):
        assert score(**{name: None}) != 0 and "scores, counts or status is NULL" in err()


def test_python_surface_refuses_bad_parameters_before_any_gpu_work():
    from b2s_hip import f0
    import hyperparams
    hyperparams.hparams.override_from_dict(hyperparams.DEFAULTS)
    p = f0.yin_params()
    assert (p["win"], p["hop"], p["tau_min"], p["tau_max"], p["threshold"], p["sr"]) == (800, 200, 32, 266, 0.1, 16000.0)
    assert p["min_energy"] == R.min_energy(800, -40) == int(math.ceil(800 * (32767.0 * 10.0 ** (-40 / 20.0)) ** 2))
    assert type(p["min_energy"]) is int and f0.yin_params(silence_db=None)["min_energy"] == 0
    for bad in (dict(win=1), dict(win=2049), dict(hop=0), dict(tau_min=1), dict(tau_max=513), dict(tau_min=40, tau_max=40),
                dict(threshold=0.0), dict(sr=0.0), dict(fmin=10.0), dict(fmin=600.0), dict(fmax=16000.0), dict(silence_db=200.0)):
        with pytest.raises(f0.B2SError):
            f0.yin_params(**bad)


def test_there_is_no_cpu_fallback(monkeypatch):
    import torch
    from b2s_hip import f0
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    x = np.zeros((1, 5, 80), np.float32)
    with pytest.raises(f0.B2SError, match="runs on the GPU only"):
        f0.f0_dtw_batch(x, [5], x, [5])
    with pytest.raises(f0.B2SError, match="runs on the GPU only"):
        f0.f0(np.zeros(400, np.float32))
    with pytest.raises(f0.B2SError, match="runs on the GPU only"):
        f0.quantize_batch(np.zeros((1, 400), np.float32), [400])


def test_command_line_usage_errors_are_nonzero(tmp_path, capsys):
    import hyperparams
    from b2s_hip import f0
    hyperparams.hparams.override_from_dict(hyperparams.DEFAULTS)
    assert f0.main([str(tmp_path / "nowhere"), "--data-dir", str(tmp_path)]) == 2
    assert f0.main([str(tmp_path), "--data-dir", str(tmp_path)]) == 2                  # no mels.zip there
    assert f0.main([str(tmp_path), "--data-dir", str(tmp_path), "--radius", "0"]) == 2
    assert f0.main([str(tmp_path), "--data-dir", str(tmp_path), "--batch", "0"]) == 2
    assert f0.main([str(tmp_path), "--data-dir", str(tmp_path), "--n-iter", "-1"]) == 2
    assert f0.main([str(tmp_path), "--data-dir", str(tmp_path), "--fmin", "20"]) == 2   # tau_max = 800 > 512
    assert "tau_max <= 512" in capsys.readouterr().err
    assert f0.main([str(tmp_path), "--data-dir", str(tmp_path), "--fmin", "500", "--fmax", "400"]) == 2
    assert f0.main([str(tmp_path), "--data-dir", str(tmp_path), "--threshold", "0"]) == 2
    with pytest.raises(SystemExit) as e:
        f0.main([])
    assert e.value.code == 2
    capsys.readouterr()


# ----------------------------------------------------------------------------------------------------------------- the oracle

PRM = dict(win=800, hop=200, tau_min=32, tau_max=266)


def interior(n_frames, L, win=800, hop=200, tau_max=266):
    """Frames whose whole segment lies inside the signal."""
    half = (win + tau_max) // 2
    return [t for t in range(n_frames) if t * hop - half >= 0 and t * hop - half + win + tau_max <= L]


def periodic(P, L, seed=3):
    return np.tile(np.random.default_rng(seed).integers(-20000, 20000, P), L // P + 1)[:L].astype(np.int16)


@pytest.mark.parametrize("P", [32, 44, 100, 123, 266])
def test_an_exactly_periodic_signal_is_picked_at_its_period(P):
    """tau == P and c[P] == 0.0 over the whole lag range, its two ends included.  F0 is within 0.1 Hz of sr / P from P = 44 on.
    Below that the definition itself does not allow 0.1 Hz: with d[P] = 0 and d[P - 1] ~ d[P + 1] the normalisation leaves
    c[P + 1] / c[P - 1] ~ (P + 1) / (P - 1), so the parabola is shifted by about -1 / (2 P) lags, which is sr / (2 P^3) in Hz:
    0.24 Hz at P = 32 (0.16 Hz is what this signal gives), 0.1 Hz at P = 43.1.  There the bound is that figure."""
    pcm = periodic(P, 3000)
    out = R.yin(pcm, **PRM)
    inner = interior(len(out["tau"]), len(pcm))
    assert len(inner) >= 5
    for t in inner:
        assert out["tau"][t] == P and out["cmnd"][t, P] == 0.0 and out["aper"][t] == 0.0
        assert abs(out["f0"][t] - 16000.0 / P) <= (0.1 if P >= 44 else 16000.0 / (2 * P ** 3))


def test_zeros_and_a_constant_have_no_voiced_frame():
    for pcm in (np.zeros(3000, np.int16), np.full(3000, 12345, np.int16)):
        out = R.yin(pcm, **PRM)
        inner = interior(len(out["tau"]), len(pcm))
        assert np.all(out["cmnd"][inner] == 1.0)
        assert np.all(out["tau"] == 0) and np.all(out["f0"] == 0.0)


def test_scaling_the_pcm_by_two_leaves_c_bit_equal():
    rng = np.random.default_rng(5)
    n = np.arange(2400)
    pcm = np.rint(9000 * np.sin(2 * np.pi * n / 77.3) + 2000 * rng.standard_normal(len(n))).astype(np.int16)
    assert np.abs(pcm).max() < 16384
    a, b = R.yin(pcm, **PRM), R.yin((2 * pcm).astype(np.int16), **PRM)
    assert np.array_equal(a["cmnd"].view(np.int64), b["cmnd"].view(np.int64))
    assert np.array_equal(a["tau"], b["tau"]) and np.array_equal(a["f0"], b["f0"]) and a["tau"].max() > 0


def test_the_largest_difference_function_stays_inside_the_exact_range():
    """A full-scale square wave at the stated maxima: d below 2^43, its running sum and d * tau below 2^53."""
    n = np.arange(2048 + 512)
    seg = np.where((n // 61) % 2 == 0, 32767, -32768).astype(np.int64)
    d = R.difference(seg, 2048, 512)
    assert d.dtype == np.int64 and 0 < int(d.max()) < 2 ** 43
    assert int(np.cumsum(d)[-1]) < 2 ** 53 and int((d * np.arange(513)).max()) < 2 ** 53
    brute = [sum((int(seg[j]) - int(seg[j + tau])) ** 2 for j in range(2048)) for tau in (0, 1, 61, 512)]
    assert [int(d[tau]) for tau in (0, 1, 61, 512)] == brute


def test_silence_floor_is_an_integer_comparison():
    pcm = periodic(100, 3000)
    out = R.yin(pcm, **PRM)
    t = interior(len(out["tau"]), len(pcm))[0]
    e = out["energy"][t]
    assert R.yin(pcm, floor=e, **PRM)["tau"][t] == 100 and R.yin(pcm, floor=e + 1, **PRM)["tau"][t] == 0


def test_the_score_of_a_track_against_itself_is_zero():
    out = R.yin(periodic(100, 3000), **PRM)
    out["tau"][3] = 0
    F = len(out["tau"])
    kept = np.arange(F)
    path = [(i, i) for i in range(F)]
    s = R.score(out["f0"], out["tau"], out["f0"], out["tau"], kept, kept, path)
    assert s["status"] == R.OK and s["counts"][0] == F and s["counts"][1] == 0 and s["counts"][2] > 0 and s["counts"][3] == 0
    assert s["scores"] == [0.0, 0.0, 0.0, 0.0, 0.0]


def test_score_counts_in_closed_form():
    f0x, taux = np.array([100.0, 0.0, 200.0, 125.0, 0.0]), np.array([160, 0, 80, 128, 0])
    f0y, tauy = np.array([100.0, 110.0, 100.0, 0.0]), np.array([160, 145, 160, 0])
    kept_x, kept_y = [0, 2, 3, 4], [0, 1, 2, 3]
    path = [(0, 0), (1, 1), (1, 2), (2, 2), (2, 3), (3, 3)]     # 100/100, 200/110, 200/100, 125/100, 125/-, -/-
    s = R.score(f0x, taux, f0y, tauy, kept_x, kept_y, path)
    assert s["counts"] == [6, 1, 4, 3]
    want_hz = math.sqrt((0 + 90.0 ** 2 + 100.0 ** 2 + 25.0 ** 2) / 4)
    assert abs(s["scores"][0] - want_hz) <= 1e-12 * want_hz
    assert s["scores"][2:] == [1 / 6, 3 / 4, 4 / 6]
    assert R.score(f0x, taux, f0y, tauy, kept_x, kept_y, [])["status"] == R.EMPTY
    assert R.score(f0x, taux, f0y, tauy, kept_x, kept_y, [(4, 0)])["status"] == R.FAILED
    assert R.score(f0x, taux, f0y, tauy, [0, 2, 3, 5], kept_y, [(3, 0)])["status"] == R.FAILED
    none = R.score(f0x, taux, f0y, tauy, kept_x, kept_y, [(3, 0), (0, 3)])
    assert none["counts"] == [2, 2, 0, 0] and math.isnan(none["scores"][0]) and math.isnan(none["scores"][3])
    assert none["scores"][2] == 1.0 and none["scores"][4] == 1.0


def test_quantiser_is_the_rule_of_save_wav(tmp_path):
    import wave
    import types
    from b2s_hip import vocoder
    rng = np.random.default_rng(2)
    for scale in (3.7, 0.3, 0.001):
        wav = (scale * rng.standard_normal(500)).astype(np.float32)
        path = vocoder.save_wav(wav, str(tmp_path / "a.wav"), types.SimpleNamespace(sr=16000))
        with wave.open(path, "rb") as w:
            written = np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")
        pcm, peak, status = R.quantize(wav)
        assert status == R.OK and np.array_equal(pcm, written) and peak == np.abs(wav).max()
    assert R.quantize(np.array([0.1, np.nan], np.float32))[2] == R.FAILED
    assert R.quantize(np.zeros(0, np.float32))[2] == R.OK
