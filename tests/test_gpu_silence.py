"""The batched GPU silence splitting / trimming (b2s_hip.vocoder, csrc/vocoder/silence.hip) against the fp64 restatement of librosa
0.6.0's effects.split / effects.trim (tests/silence_ref.py), on the fixture batch of silence_ref.fixture_batch() and for the three
parameter sets the reference uses.

Everything is compared exactly and no frame is excluded: tests/test_silence_host.py asserts that no frame of the fixture lies within
1e-3 dB of the threshold, 100 x what the fp32 frame energy can be off by.  Only the end-to-end test, whose waveforms come out of the
GPU vocoder and are not chosen by the fixture, may leave out an utterance with such a frame -- one at most; it prints how many it
left out."""
import logging
import wave

import numpy as np
import pytest
import torch

import audio_ref as A
import silence_ref as R

pytestmark = pytest.mark.gpu


def fresh_hp(over=""):
    import hyperparams
    hp = hyperparams.hparams
    hp.override_from_dict(hyperparams.DEFAULTS)
    if over:
        hp.parse(over)
    return hp


def padded(ws):
    pad = np.zeros((len(ws), max(len(w) for w in ws)), np.float32)
    for i, w in enumerate(ws):
        pad[i, :len(w)] = w
    return torch.from_numpy(pad).cuda(), [len(w) for w in ws]


def kept(w, params):
    return np.concatenate([w[l:r] for l, r in R.split(w, *params)])


def check_against_restatement(ws, params):
    from b2s_hip import vocoder
    dev, lens = padded(ws)
    iv, flags = vocoder.split_batch(dev, lens, *params, return_flags=True)
    trim = vocoder.trim_batch(dev, lens, *params)
    out, out_lens = vocoder.remove_silence_batch(dev, lens, *params)
    assert out.shape == dev.shape and out.dtype == torch.float32 and trim.shape == (len(ws), 2)
    out = out.cpu().numpy()
    for b, w in enumerate(ws):
        np.testing.assert_array_equal(flags[b], R.nonsilent(w, *params), err_msg="flags of utterance %d (L=%d)" % (b, len(w)))
        want = R.split(w, *params)
        assert iv[b].dtype == np.int64 and iv[b].shape == want.shape, (len(w), iv[b], want)
        np.testing.assert_array_equal(iv[b], want)
        np.testing.assert_array_equal(trim[b], R.trim_index(w, *params))
        want_wav = kept(w, params)
        assert out_lens[b] == len(want_wav)
        assert np.array_equal(out[b, :out_lens[b]].view(np.uint32), want_wav.view(np.uint32)), len(w)
        assert not np.any(out[b, out_lens[b]:]), "samples past out_lengths must be zero"


@pytest.mark.parametrize("params", R.PARAM_SETS)
def test_fixture_batch_matches_the_restatement_exactly(params):
    check_against_restatement(R.fixture_batch(), params)


@pytest.mark.parametrize("params", [(40, 300, 70), (35, 301, 301), (60, 2, 1), (30, 8192, 8192), (45, 8192, 3000)])
def test_parameter_sets_off_the_sliding_path(params):
    """frame_length % hop != 0 (direct per-frame sums), an odd frame_length, and the ends of the accepted range."""
    ws = R.fixture_batch()[:8]
    for w in ws:
        assert R.frames_in_band(w, *params)[0] == 0
    check_against_restatement(ws, params)


def test_edge_cases_on_the_device():
    rng = np.random.default_rng(3)
    tone = (0.4 * np.sin(np.arange(5000) * 0.05)).astype(np.float32)
    ws = [np.zeros(4000, np.float32),                        # all-zero: one interval [0, L]
          np.zeros(2, np.float32),
          tone[:150].copy(),                                 # L < hop (200) and L < frame_length // 2 (3200): repeated reflection
          tone[:2].copy(),
          np.concatenate([np.zeros(1037 - 537, np.float32), tone[:537]]),      # L not a multiple of hop, interval clipped to L
          (tone * (rng.random(5000) > 0.5)).astype(np.float32)]
    from b2s_hip import vocoder
    for params in R.PARAM_SETS + [(40, 300, 70)]:
        for w in ws:
            assert R.frames_in_band(w, *params)[0] == 0
        check_against_restatement(ws, params)
    dev, lens = padded(ws)
    iv = vocoder.split_batch(dev, lens, *R.TRIM_PARAMS)
    np.testing.assert_array_equal(iv[0], [[0, 4000]])
    np.testing.assert_array_equal(iv[2], [[0, 150]])
    # the single-utterance functions with the reference's signatures
    y = R.fixture_batch()[7]
    np.testing.assert_array_equal(vocoder.effects_split(y, 40, 256, 64), R.split(y, 40, 256, 64))
    got, idx = vocoder.effects_trim(y, top_db=40, frame_length=256, hop_length=64)
    np.testing.assert_array_equal(idx, R.trim_index(y, 40, 256, 64))
    np.testing.assert_array_equal(got, R.trim(y, 40, 256, 64)[0])
    fresh_hp()
    one = vocoder.trim_silence_intervals(y)
    assert one.dtype == np.float32 and np.array_equal(one, R.trim_silence_intervals(y))


def test_bit_identical_across_runs_and_independent_of_the_batch():
    from b2s_hip import vocoder
    ws = R.fixture_batch()
    dev, lens = padded(ws)
    for params in R.PARAM_SETS:
        a = vocoder._split_device(dev, lens, *params, want_flags=True)
        b = vocoder._split_device(dev, lens, *params, want_flags=True)
        wa, wb = vocoder._gather_device(a), vocoder._gather_device(b)
        torch.cuda.synchronize()
        n = a["n"].cpu().numpy()
        assert torch.equal(a["n"], b["n"]) and torch.equal(a["trim"], b["trim"]) and torch.equal(a["out_lengths"], b["out_lengths"])
        assert torch.equal(wa, wb)
        for i in range(len(ws)):
            assert torch.equal(a["intervals"][i, :n[i]], b["intervals"][i, :n[i]])
            assert torch.equal(a["flags"][i, :a["frames"][i]], b["flags"][i, :a["frames"][i]])
        for i in (0, 4, 8, 10):
            one = vocoder._split_device(dev[i:i + 1, :lens[i]].contiguous(), [lens[i]], *params, want_flags=True)
            w1 = vocoder._gather_device(one)
            assert int(one["n"][0]) == n[i]
            assert torch.equal(one["intervals"][0, :n[i]], a["intervals"][i, :n[i]])
            assert torch.equal(one["flags"][0, :one["frames"][0]], a["flags"][i, :a["frames"][i]])
            assert torch.equal(one["trim"][0], a["trim"][i]) and torch.equal(one["out_lengths"][0], a["out_lengths"][i])
            assert torch.equal(w1[0], wa[i, :lens[i]])


def _read_wav(path):
    with wave.open(path, "rb") as w:
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2")


def test_save_eval_results_writes_trimmed_waves_on_the_gpu(tmp_path, caplog):
    import synthesize
    from b2s_hip import vocoder
    fresh_hp()
    sigs = [w for w in R.fixture_batch() if len(w) >= 200]       # at least 2 mel frames: what the vocoder accepts
    mels = [A.get_spectrograms(w) for w in sigs]
    lengths = [m.shape[0] for m in mels]
    names = ["u%d" % i for i in range(len(sigs))]
    mel_aft = np.zeros((len(sigs), max(lengths), 80), np.float32)
    for i, m in enumerate(mels):
        mel_aft[i, :lengths[i]] = m
    out = tmp_path / "o"
    fresh_hp("vocoder=hip,trim=hip,n_iter=3")
    try:
        synthesize.save_eval_results(names, mel_aft, mel_aft, {"encdec": []}, [5] * len(names), lengths, str(out), save_trimmed_wave=True,
                                     n_plot_alignment=0)
        wav, lens = vocoder.mel2wav_batch(mel_aft, lengths)
        wav = wav.cpu().numpy()
        left_out = []
        for i, name in enumerate(names):
            w = wav[i, :lens[i]]
            assert (out / ("%s.wav" % name)).exists() and (out / ("%s_trim.wav" % name)).exists()
            if R.frames_in_band(w, *R.TRIM_PARAMS)[0] > 0:
                left_out.append(name)
                continue
            vocoder.save_wav(R.trim_silence_intervals(w), str(tmp_path / "want.wav"))
            got, want = _read_wav(str(out / ("%s_trim.wav" % name))), _read_wav(str(tmp_path / "want.wav"))
            assert got.shape == want.shape and np.array_equal(got, want), name
        print("end to end: %d of %d utterances left out as near-threshold: %s" % (len(left_out), len(names), left_out))
        assert len(left_out) <= 1, left_out
    finally:
        fresh_hp()
    # trim=reference: the parent's behaviour -- a warning, and no _trim.wav unless the reference's librosa path is importable
    try:
        from utils.audio import trim_silence_intervals  # noqa: F401
        have_ref = True
    except Exception:
        have_ref = False
    fresh_hp("vocoder=hip,n_iter=1")
    try:
        with caplog.at_level(logging.WARNING):
            synthesize.save_eval_results(names[:2], mel_aft[:2], mel_aft[:2], {"encdec": []}, [5, 5], lengths[:2], str(tmp_path / "r"),
                                         save_trimmed_wave=True, n_plot_alignment=0)
        assert (tmp_path / "r" / "u0.wav").exists()
        assert (tmp_path / "r" / "u0_trim.wav").exists() == have_ref
        assert any("trimmed waves need the reference" in r.getMessage() for r in caplog.records) == (not have_ref)
    finally:
        fresh_hp()


def test_errors_raise_b2s_error():
    from b2s_hip import B2SError, vocoder
    z = torch.zeros(2, 400, device="cuda")
    with pytest.raises(B2SError, match="frame_length must be in 2..8192"):
        vocoder.split_batch(z, [400, 300], 40, 9000, 64)
    with pytest.raises(B2SError, match="hop_length must be in 1..frame_length"):
        vocoder.split_batch(z, [400, 300], 40, 256, 0)
    with pytest.raises(B2SError, match="top_db must be > 0"):
        vocoder.split_batch(z, [400, 300], 0, 256, 64)
    with pytest.raises(B2SError, match="2..Lmax"):
        vocoder.split_batch(z, [400, 1], 40, 256, 64)
