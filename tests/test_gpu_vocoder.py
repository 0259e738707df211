"""The batched GPU Griffin-Lim vocoder and mel front end (b2s_hip.vocoder, libb2s_vocoder.so) against the fp64 restatement of the
reference's utils/audio.py (tests/audio_ref.py), on one seeded ragged batch with T in {2, 3, 6, 7, 64, 1000, 1100}.

Griffin-Lim's phase projection is ill-conditioned where |est| is near zero, so fp32 rounding moves the waveform far more than the
spectral convergence: the wav gates are loose, the spectral-convergence gate is tight.  Each gate is min(the cap, 2 x the value
measured on an MI355X (profiles/r07_vocoder_accuracy.json), except where noted at GATES."""
import os
import wave

import numpy as np
import pytest
import torch

import audio_ref as A

pytestmark = pytest.mark.gpu

TS = [2, 3, 6, 7, 64, 1000, 1100]
# per n_iter: (spectral convergence relative to the oracle's, magnitude-spectrogram rel. L2, wav rel. L2).  Caps 1e-2 / 2e-2 / 5e-2;
# worst measured (n_iter 1 / 5 / 60): sc 1.3e-4 / 2.3e-4 / 6.2e-4, mag 6.1e-3 / 1.7e-2 / 3.9e-2, wav 7.5e-4 / 2.5e-3 / 1.25e-2.
# The magnitude gate at 60 iterations is 2 x the measurement, above its cap: an all-fp32 NumPy (pocketfft) Griffin-Lim lands at
# 2.9e-2 on the same utterance, so no fp32 vocoder meets 2e-2 there (profiles/r07_vocoder_accuracy.json).
GATES = {1: (2.6e-4, 1.2e-2, 1.5e-3), 5: (4.7e-4, 2e-2, 5e-3), 60: (1.25e-3, 8e-2, 2.5e-2)}
WAV0_GATE = 1e-5              # measured 9.8e-6 (T = 2), 3e-6 to 4.4e-6 for the others
WAV2MEL_GATE = 4e-5           # measured 9.1e-6 max abs on the batch's waveforms


def fresh_hp(over=""):
    import hyperparams
    hp = hyperparams.hparams
    hp.override_from_dict(hyperparams.DEFAULTS)
    if over:
        hp.parse(over)
    return hp


def _signal(n, seed):
    """Voiced-like test signal: a gliding harmonic series plus a noise floor (keeps every mel bin well above the -100 dB floor)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    f0 = 110.0 + 60.0 * np.sin(2 * np.pi * 0.7 * t + seed)
    ph = 2 * np.pi * np.cumsum(f0) / 16000.0
    y = sum(0.3 / h * np.sin(h * ph) for h in range(1, 12))
    return (y + 0.03 * rng.standard_normal(n)).astype(np.float32)


@pytest.fixture(scope="module")
def batch():
    fresh_hp()
    wavs = [_signal(200 * (T - 1), 11 + i) for i, T in enumerate(TS)]
    mels = [A.get_spectrograms(w) for w in wavs]
    assert [m.shape[0] for m in mels] == TS
    pad = np.zeros((len(TS), max(TS), 80), np.float32)
    for i, m in enumerate(mels):
        pad[i, :m.shape[0]] = m
    return {"wavs": wavs, "mels": mels, "pad": pad}


_oracle_cache = {}


def oracle(batch, n_iter):
    if n_iter not in _oracle_cache:
        _oracle_cache[n_iter] = [A.mel2wav(m, n_iter=n_iter, return_raw=True) for m in batch["mels"]]
    return _oracle_cache[n_iter]


def gpu_batch(batch, n_iter):
    from b2s_hip import vocoder
    fresh_hp()
    wav, lens = vocoder.mel2wav_batch(torch.from_numpy(batch["pad"]).cuda(), TS, n_iter=n_iter)
    torch.cuda.synchronize()
    assert lens == [200 * (T - 1) for T in TS]
    assert wav.shape == (len(TS), 200 * (max(TS) - 1)) and wav.dtype == torch.float32
    w = wav.cpu().numpy()
    for i, L in enumerate(lens):
        assert not np.any(w[i, L:]), "padding past L_b must be zero"
    return [w[i, :L] for i, L in enumerate(lens)]


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def pre(w):
    """Undo the de-emphasis exactly: y before lfilter."""
    w = np.asarray(w, np.float64)
    return np.append(w[0], w[1:] - A.PREEMPH * w[:-1])


def test_no_iterations_is_istft_plus_deemphasis(batch):
    got = gpu_batch(batch, 0)
    for i, T in enumerate(TS):
        want = oracle(batch, 0)[i][0]
        assert got[i].shape == (200 * (T - 1),)
        assert rel(got[i], want) <= WAV0_GATE, (T, rel(got[i], want))


def test_griffin_lim_converges_like_the_oracle(batch):
    sc_prev = None
    for n_iter in (1, 5, 60):
        g_sc, g_mag, g_wav = GATES[n_iter]
        got = gpu_batch(batch, n_iter)
        sc = []
        for i, T in enumerate(TS):
            wav_r, y_r, S = oracle(batch, n_iter)[i]
            y_g = pre(got[i])
            sc_g, sc_r = A.spectral_convergence(y_g, S), A.spectral_convergence(y_r, S)
            assert abs(sc_g - sc_r) <= g_sc * sc_r, (n_iter, T, sc_g, sc_r)
            m = rel(np.abs(A.stft(y_g)), np.abs(A.stft(y_r)))
            assert m <= g_mag, (n_iter, T, m)
            wr = rel(got[i], wav_r)
            assert wr <= g_wav, (n_iter, T, wr)
            sc.append(sc_g)
        if sc_prev is not None:
            assert all(a <= b * (1 + 1e-6) for a, b in zip(sc, sc_prev)), (n_iter, sc, sc_prev)
        sc_prev = sc


def test_deterministic_and_independent_of_the_batch(batch):
    from b2s_hip import vocoder
    fresh_hp()
    mels = torch.from_numpy(batch["pad"]).cuda()
    a, _ = vocoder.mel2wav_batch(mels, TS, n_iter=5)
    b, _ = vocoder.mel2wav_batch(mels, TS, n_iter=5)
    assert torch.equal(a, b)
    for i in (0, 3, 5):
        T = TS[i]
        one, lens = vocoder.mel2wav_batch(mels[i:i + 1, :T].contiguous(), [T], n_iter=5)
        assert torch.equal(one[0, :lens[0]], a[i, :lens[0]]), T


def test_wav2mel_matches_get_spectrograms(batch):
    from b2s_hip import vocoder
    fresh_hp()
    wl = [len(w) for w in batch["wavs"]] + [1001, 257]
    ws = batch["wavs"] + [_signal(1001, 3), _signal(257, 4)]
    pad = np.zeros((len(ws), max(wl)), np.float32)
    for i, w in enumerate(ws):
        pad[i, :len(w)] = w
    mels, frames = vocoder.wav2mel_batch(torch.from_numpy(pad).cuda(), wl)
    assert frames == [1 + n // 200 for n in wl]
    m = mels.cpu().numpy()
    for i, w in enumerate(ws):
        want = A.get_spectrograms(w)
        assert want.shape[0] == frames[i]
        err = float(np.abs(m[i, :frames[i]] - want).max())
        assert err <= WAV2MEL_GATE, (wl[i], err)
        assert not np.any(m[i, frames[i]:])
    one = vocoder.get_spectrograms(ws[2])
    assert one.dtype == np.float32 and np.array_equal(one, m[2, :frames[2]])


def test_numpy_mel2wav_equals_the_batch_row(batch):
    from b2s_hip import vocoder
    fresh_hp()
    wav, lens = vocoder.mel2wav_batch(batch["pad"], TS)
    for i in (1, 4):
        one = vocoder.mel2wav(batch["mels"][i])
        assert one.dtype == np.float32 and one.shape == (200 * (TS[i] - 1),)
        assert np.array_equal(one, wav[i, :lens[i]].cpu().numpy())


def _read_wav(path):
    with wave.open(path, "rb") as w:
        return w.getnframes(), np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")


def test_save_eval_results_with_the_hip_vocoder(batch, tmp_path):
    import synthesize
    from b2s_hip import vocoder
    names = ["u0", "u1", "one", "u3"]
    lengths = [64, 7, 1, 3]
    mel_aft = np.stack([batch["mels"][4]] * 4)                  # [4, 64, 80]
    mel_aft[1, :7] = batch["mels"][3]
    mel_aft[3, :3] = batch["mels"][1]
    fresh_hp("vocoder=hip")
    try:
        synthesize.save_eval_results(names, mel_aft, mel_aft, {"encdec": []}, [5] * 4, lengths, str(tmp_path / "o"), n_plot_alignment=0)
        ok = [0, 1, 3]
        pad = np.zeros((3, 64, 80), np.float32)
        for j, i in enumerate(ok):
            pad[j, :lengths[i]] = mel_aft[i, :lengths[i]]
        wav, lens = vocoder.mel2wav_batch(pad, [lengths[i] for i in ok])
        wav = wav.cpu().numpy()
        for j, i in enumerate(ok):
            n, got = _read_wav(str(tmp_path / "o" / ("%s.wav" % names[i])))
            assert n == 200 * (lengths[i] - 1)
            vocoder.save_wav(wav[j, :lens[j]], str(tmp_path / "want.wav"))
            assert np.array_equal(got, _read_wav(str(tmp_path / "want.wav"))[1])
        for nm in names:
            assert (tmp_path / "o" / ("%s.npy" % nm)).exists()
        assert not (tmp_path / "o" / "one.wav").exists()        # T = 1: logged and skipped, the others are written
    finally:
        fresh_hp()
    # the default keeps today's behaviour: wavs only through the reference's utils.audio
    try:
        import utils.audio  # noqa: F401
        have_ref = True
    except Exception:
        have_ref = False
    synthesize.save_eval_results(names[:1], mel_aft[:1], mel_aft[:1], {"encdec": []}, [5], lengths[:1], str(tmp_path / "d"), n_plot_alignment=0)
    assert (tmp_path / "d" / "u0.npy").exists()
    assert (tmp_path / "d" / "u0.wav").exists() == have_ref


def test_errors_raise_b2s_error():
    from b2s_hip import B2SError, vocoder
    fresh_hp()
    with pytest.raises(B2SError, match="HIP device"):
        vocoder.mel2wav_batch(torch.zeros(1, 4, 80), [4])
    with pytest.raises(B2SError, match="n_fft=2048"):
        vocoder.mel2wav_batch(torch.zeros(1, 4, 80, device="cuda"), [4], hp=fresh_hp("n_fft=1024"))
    fresh_hp()
    with pytest.raises(B2SError, match="2..Tmax"):
        vocoder.mel2wav_batch(torch.zeros(2, 4, 80, device="cuda"), [4, 1])


def test_full_size_batch_is_finite():
    from b2s_hip import vocoder
    fresh_hp()
    g = torch.Generator(device="cuda").manual_seed(5)
    mels = (torch.rand(64, 1000, 80, device="cuda", generator=g) * 6 - 4).contiguous()
    wav, lens = vocoder.mel2wav_batch(mels, [1000] * 64, n_iter=60)
    torch.cuda.synchronize()
    assert wav.shape == (64, 199800) and lens == [199800] * 64
    assert bool(torch.isfinite(wav).all())
