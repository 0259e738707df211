"""CPU-only tests of the vocoder's host side: the mel basis, the fp64 restatement (tests/audio_ref.py) that the GPU tests compare
against, the libb2s_vocoder.so C ABI (exports, argument errors without a GPU), save_wav and the `vocoder` hyper-parameter."""
import ctypes as C
import os
import re
import wave

import numpy as np
import pytest

import audio_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fresh_hp(over=""):
    import hyperparams
    hp = hyperparams.hparams
    hp.override_from_dict(hyperparams.DEFAULTS)
    if over:
        hp.parse(over)
    return hp


def _slaney_mel(f):
    """Element-wise Slaney scale: 3 mels per 200 Hz below 1 kHz, then log steps of ln(6.4)/27."""
    return f / (200.0 / 3) if f < 1000.0 else 15.0 + np.log(f / 1000.0) / (np.log(6.4) / 27.0)


def _slaney_hz(m):
    return m * (200.0 / 3) if m < 15.0 else 1000.0 * np.exp((m - 15.0) * np.log(6.4) / 27.0)


def test_mel_basis_matches_elementwise_slaney_formula():
    from b2s_hip import vocoder
    hp = fresh_hp()
    basis = vocoder.mel_basis(hp)
    assert basis.shape == (80, 1025) and basis.dtype == np.float64
    top = _slaney_mel(8000.0)
    pts = [_slaney_hz(top * i / 81) for i in range(82)]
    freqs = [8000.0 * k / 1024 for k in range(1025)]
    ref = np.zeros((80, 1025))
    for i in range(80):
        lo, c, hi = pts[i], pts[i + 1], pts[i + 2]
        for k, f in enumerate(freqs):
            ref[i, k] = max(0.0, min((f - lo) / (c - lo), (hi - f) / (hi - c))) * 2.0 / (hi - lo)
    np.testing.assert_allclose(basis, ref, rtol=1e-9, atol=1e-15)
    np.testing.assert_array_equal(basis, A.mel_basis())
    # triangles peak at the bin nearest their mel centre, never above 2 / width, and carry unit area over frequency (norm=1)
    for i in range(80):
        near = int(np.argmin(np.abs(np.array(freqs) - pts[i + 1])))
        assert abs(int(np.argmax(basis[i])) - near) <= 1
        assert basis[i].max() <= 2.0 / (pts[i + 2] - pts[i]) + 1e-15
        assert abs(np.trapezoid(basis[i], freqs) - 1.0) < 0.03, i
    inv = vocoder.inverse_mel_basis(hp)
    assert inv.shape == (1025, 80)
    np.testing.assert_allclose(basis @ inv, np.eye(80), atol=1e-8)


def test_restatement_istft_inverts_stft():
    rng = np.random.default_rng(0)
    for T in (2, 3, 7, 40):
        y = rng.standard_normal(200 * (T - 1))
        X = A.stft(y)
        assert X.shape == (1025, T)
        np.testing.assert_allclose(A.istft(X), y, atol=1e-10, rtol=0)


@pytest.mark.parametrize("T", [2, 3, 6, 7])
def test_reflect_index_equals_numpy_pad(T):
    L = 200 * (T - 1)
    y = np.arange(L, dtype=np.float64) * 1.5 + 3.0
    want = np.pad(y, 1024, mode="reflect")
    got = y[A.reflect_index(np.arange(-1024, L + 1024), L)]
    np.testing.assert_array_equal(got, want)
    assert A.stft(y).shape[1] == T


def test_vocoder_library_exports_every_declared_symbol():
    from b2s_hip import vocoder
    l = vocoder.load()
    header = open(os.path.join(ROOT, "include", "b2s_vocoder.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(b2s_voc_[a-z0-9_]+)\s*\(", header))
    assert declared == set(vocoder.EXPORTS), declared ^ set(vocoder.EXPORTS)
    for name in sorted(declared):
        assert hasattr(l, name)
    assert l.b2s_voc_version() >= 100
    # the model library's ABI is unchanged: no vocoder entry point there
    from b2s_hip import lib
    assert not any(n.startswith("b2s_voc") for n in lib.EXPORTS)


def test_argument_errors_come_back_as_messages_without_a_gpu():
    from b2s_hip import vocoder
    l = vocoder.load()
    hp = fresh_hp()
    p = vocoder.params(hp)
    assert l.b2s_voc_ws_bytes(C.byref(p), 2, 10, 5, vocoder.WS_MEL2WAV) > 10 * 1025 * 4
    bad = vocoder.params(fresh_hp("n_fft=1024"))
    assert l.b2s_voc_mel2wav(C.byref(bad), None, None, 2, 5, 10, 60, None, None, None, 0, None) != 0
    msg = l.b2s_voc_last_error().decode()
    assert "n_fft=1024" in msg and "n_fft=2048" in msg and "win_length=800" in msg and "hop_length=200" in msg
    assert l.b2s_voc_ws_bytes(C.byref(bad), 2, 10, 5, vocoder.WS_WAV2MEL) == 0 and b"n_fft=2048" in l.b2s_voc_last_error()
    assert l.b2s_voc_mel2wav(C.byref(p), None, None, 0, 5, 10, 60, None, None, None, 0, None) != 0
    assert b"B must be > 0" in l.b2s_voc_last_error()
    assert l.b2s_voc_mel2wav(C.byref(p), None, None, 2, 5, 11, 60, None, None, None, 0, None) != 0
    assert b"total_frames 11 does not match" in l.b2s_voc_last_error()
    assert l.b2s_voc_wav2mel(C.byref(p), None, None, None, 2, 400, 7, None, None, None, 0, None) != 0
    assert b"total_frames 7 does not match" in l.b2s_voc_last_error()
    assert l.b2s_voc_mel2wav(C.byref(p), None, None, 2, 5, 10, -1, None, None, None, 0, None) != 0
    assert b"n_iter" in l.b2s_voc_last_error()
    assert l.b2s_voc_mel2wav(C.byref(p), None, None, 2, 5, 10, 60, None, None, None, 0, None) != 0
    assert b"NULL" in l.b2s_voc_last_error()
    fresh_hp()


def test_batch_calls_refuse_cpu_tensors_and_bad_lengths():
    import torch
    from b2s_hip import B2SError, vocoder
    fresh_hp()
    with pytest.raises(B2SError, match="HIP device"):
        vocoder.mel2wav_batch(torch.zeros(2, 5, 80), [5, 3])
    with pytest.raises(B2SError, match="HIP device"):
        vocoder.wav2mel_batch(torch.zeros(2, 400), [400, 300])


def test_save_wav_scales_and_writes_16bit_pcm(tmp_path):
    from b2s_hip import vocoder
    fresh_hp()
    wav = np.array([0.0, 0.25, -0.5, 0.1, 0.5], dtype=np.float32)
    path = str(tmp_path / "a.wav")
    vocoder.save_wav(wav, path)
    with wave.open(path, "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 16000, 5)
        got = np.frombuffer(w.readframes(5), dtype="<i2")
    np.testing.assert_array_equal(got, np.round(np.clip(wav / 0.5, -1, 1) * 32767).astype(np.int16))
    quiet = np.array([0.001, -0.004], dtype=np.float32)          # peak below 0.01: scaled by 1 / 0.01, not to full scale
    vocoder.save_wav(quiet, path)
    with wave.open(path, "rb") as w:
        got = np.frombuffer(w.readframes(2), dtype="<i2")
    np.testing.assert_array_equal(got, np.round(quiet / 0.01 * 32767).astype(np.int16))


def test_vocoder_hparam_defaults_to_reference():
    import hyperparams
    hp = fresh_hp()
    assert hp.vocoder == "reference" and hyperparams.DEFAULTS["vocoder"] == "reference"
    hp.parse("vocoder=hip")
    assert hp.vocoder == "hip"
    fresh_hp()


def test_unknown_vocoder_is_refused(tmp_path):
    import synthesize
    fresh_hp("vocoder=griffin")
    try:
        with pytest.raises(ValueError, match="unknown vocoder"):
            synthesize.save_eval_results(["a"], None, np.zeros((1, 4, 80), np.float32), {"encdec": []}, [3], [4], str(tmp_path))
    finally:
        fresh_hp()
