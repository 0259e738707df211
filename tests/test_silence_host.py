"""CPU-only tests of the silence splitting / trimming host side: the fp64 restatement (tests/silence_ref.py) against cases whose
intervals follow by hand from the frame geometry, the new libb2s_vocoder.so entry points (declared, exported, bound; argument errors
without a GPU), the `trim` hyper-parameter, and the precondition of the GPU parity tests' fixture.

Geometry used by the hand-derived cases: with pad = frame_length // 2, frame f covers the samples [f * hop - pad, f * hop - pad +
frame_length).  For a constant-amplitude burst on an exact-zero floor that is longer than frame_length + hop and further than pad from
both ends, some frame lies wholly inside the burst, so a frame's level is 10 log10(overlap / frame_length) dB; for the three parameter
sets frame_length * 10 ** (-top_db / 10) < 1, so a frame is non-silent exactly when it overlaps the burst by at least one sample."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import silence_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["b2s_voc_silence_gather", "b2s_voc_silence_split", "b2s_voc_silence_ws_bytes"]


def fresh_hp(over=""):
    import hyperparams
    hp = hyperparams.hparams
    hp.override_from_dict(hyperparams.DEFAULTS)
    if over:
        hp.parse(over)
    return hp


def burst(L, s, e, amp=0.3):
    y = np.zeros(L, np.float32)
    y[s:e] = amp
    return y


def by_hand(L, s, e, frame_length, hop):
    """The one interval of a burst [s, e): first frame with f * hop - pad + frame_length > s, last frame with f * hop - pad < e."""
    pad = frame_length // 2
    first = (s + pad - frame_length) // hop + 1
    last = -((-(e + pad)) // hop) - 1
    return [max(first, 0) * hop, min(L, (last + 1) * hop)]


@pytest.mark.parametrize("params,want", [((50, 6400, 200), [9200, 28200]), ((40, 2048, 512), [11776, 26112]),
                                         ((40, 256, 64), [12224, 25152])])
def test_burst_on_a_zero_floor_gives_the_interval_derived_by_hand(params, want):
    top_db, fl, hop = params
    assert fl * 10 ** (-top_db / 10.0) < 1
    L, s, e = 40000, 12345, 25000
    assert by_hand(L, s, e, fl, hop) == want
    y = burst(L, s, e)
    np.testing.assert_array_equal(R.split(y, *params), [want])
    got, idx = R.trim(y, *params)
    np.testing.assert_array_equal(idx, want)
    np.testing.assert_array_equal(got, y[want[0]:want[1]])
    # two bursts: two intervals, each from the same geometry
    y2 = burst(L, 8000, 16000) + burst(L, 26000, 34000)
    np.testing.assert_array_equal(R.split(y2, *params), [by_hand(L, 8000, 16000, fl, hop), by_hand(L, 26000, 34000, fl, hop)])
    np.testing.assert_array_equal(R.trim_index(y2, *params), [by_hand(L, 8000, 16000, fl, hop)[0], by_hand(L, 26000, 34000, fl, hop)[1]])


@pytest.mark.parametrize("params", R.PARAM_SETS)
@pytest.mark.parametrize("L", [2, 150, 199, 200, 1000, 6401])
def test_all_zero_input_is_one_interval(params, L):
    y = np.zeros(L, np.float32)
    assert R.nonsilent(y, *params).all()                     # both terms of the level clamp to -100 dB
    np.testing.assert_array_equal(R.split(y, *params), [[0, L]])
    np.testing.assert_array_equal(R.trim_index(y, *params), [0, L])


def test_shorter_than_one_hop_is_one_frame():
    y = burst(150, 20, 60)
    assert R.frame_mse(y, 6400, 200).shape == (1,)
    np.testing.assert_array_equal(R.split(y, *R.TRIM_PARAMS), [[0, 150]])
    np.testing.assert_array_equal(R.trim_silence_intervals(y), y)


def test_length_not_a_multiple_of_hop_and_interval_clipped_to_length():
    L = 1037
    y = burst(L, 500, L)
    assert R.frame_mse(y, 256, 64).shape == (1 + L // 64,)
    # the burst runs to the end: the last frame is non-silent, its edge F * hop = 1088 is clipped to L
    assert by_hand(L, 500, L, 256, 64)[0] == 384
    np.testing.assert_array_equal(R.split(y, 40, 256, 64), [[384, L]])
    np.testing.assert_array_equal(R.trim_index(y, 40, 256, 64), [384, L])


@pytest.mark.parametrize("L,fl,hop", [(100, 256, 64), (150, 6400, 200), (150, 2048, 512), (2, 256, 64), (1000, 6400, 200), (777, 300, 70),
                                      (501, 301, 301)])
def test_frame_energy_equals_numpy_pad_framing(L, fl, hop):
    """Includes L < frame_length // 2: np.pad reflects repeatedly there, and so must the restatement's index rule."""
    rng = np.random.default_rng(L)
    y = rng.standard_normal(L)
    yp = np.pad(y, fl // 2, mode="reflect")
    F = 1 + (len(yp) - fl) // hop
    want = np.array([np.mean(yp[f * hop:f * hop + fl] ** 2) for f in range(F)])
    np.testing.assert_allclose(R.frame_mse(y, fl, hop), want, rtol=1e-13, atol=0)


def test_shorter_than_half_a_frame_reflects_repeatedly():
    y = burst(100, 90, 100, 0.5)                             # pad 128 > L - 1: frame 0 sees samples 90..99 several times
    assert R.frame_mse(y, 256, 64).shape == (2,)
    np.testing.assert_array_equal(R.split(y, 40, 256, 64), [[0, 100]])


@pytest.mark.parametrize("params", R.PARAM_SETS)
def test_trim_is_first_and_last_edge_of_split(params):
    for y in R.fixture_batch() + [burst(40000, 12345, 25000)]:
        iv = R.split(y, *params)
        assert len(iv) >= 1 and np.all(iv[:, 0] < iv[:, 1]) and np.all(iv[1:, 0] > iv[:-1, 1])
        np.testing.assert_array_equal(R.trim_index(y, *params), [iv[0, 0], iv[-1, 1]])


@pytest.mark.parametrize("params", R.PARAM_SETS)
def test_fixture_has_no_frame_near_the_threshold(params):
    """Precondition of tests/test_gpu_silence.py: an fp32 sum of <= 8192 squares in a fixed tree order is off by about 1e-6 relative,
    i.e. about 1e-5 dB; the band is 100 x that.  No frame of any fixture signal may lie inside it."""
    ws = R.fixture_batch()
    assert [len(w) for w in ws] == R.FIXTURE_LENGTHS
    counts = []
    for w in ws:
        n, nearest = R.frames_in_band(w, *params)
        assert n == 0, (len(w), nearest)
        counts.append(len(R.split(w, *params)))
    assert min(counts) >= 1 and max(counts) >= 3, counts     # the batch has both single- and multi-interval signals


def test_new_symbols_are_declared_exported_and_bound():
    from b2s_hip import vocoder
    l = vocoder.load()
    header = open(os.path.join(ROOT, "include", "b2s_vocoder.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(b2s_voc_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in vocoder.EXPORTS and name in vocoder._PROTOS
        assert getattr(l, name).argtypes == vocoder._PROTOS[name][1]
    for name in ("split_batch", "trim_batch", "trim_silence_intervals_batch", "trim_silence_intervals", "effects_split", "effects_trim"):
        assert callable(getattr(vocoder, name))
    from b2s_hip import lib
    assert not any("silence" in n for n in lib.EXPORTS)      # the model library's ABI is unchanged


def test_silence_argument_errors_come_back_as_messages_without_a_gpu():
    from b2s_hip import vocoder
    l = vocoder.load()
    err = lambda: l.b2s_voc_last_error().decode()
    assert l.b2s_voc_silence_ws_bytes(64, 199800, 6400, 200) >= 64 * 1000 * 4
    assert l.b2s_voc_silence_ws_bytes(0, 1000, 6400, 200) == 0 and "B must be > 0" in err()
    assert l.b2s_voc_silence_ws_bytes(2, 1, 6400, 200) == 0 and "Lmax must be >= 2" in err()
    for fl in (1, 8193):
        assert l.b2s_voc_silence_ws_bytes(2, 1000, fl, 1) == 0 and "frame_length must be in 2..8192" in err()
    for hop in (0, 257):
        assert l.b2s_voc_silence_ws_bytes(2, 1000, 256, hop) == 0 and "hop_length must be in 1..frame_length=256" in err()
    none = [None] * 7
    assert l.b2s_voc_silence_split(None, None, 2, 1000, 0.0, 256, 64, *none, 0, None) != 0 and "top_db must be > 0" in err()
    assert l.b2s_voc_silence_split(None, None, 2, 1000, 40.0, 256, 300, *none, 0, None) != 0 and "hop_length" in err()
    assert l.b2s_voc_silence_split(None, None, 2, 1000, 40.0, 256, 64, *none, 0, None) != 0 and "NULL" in err()
    assert l.b2s_voc_silence_gather(None, 2, 1000, 9000, 64, None, None, None, None, None, None) != 0 and "frame_length" in err()
    assert l.b2s_voc_silence_gather(None, 2, 1000, 256, 64, None, None, None, None, None, None) != 0 and "NULL" in err()


def test_silence_calls_refuse_cpu_tensors_and_bad_lengths():
    import torch
    from b2s_hip import B2SError, vocoder
    fresh_hp()
    with pytest.raises(B2SError, match="HIP device"):
        vocoder.split_batch(torch.zeros(2, 400), [400, 300])
    with pytest.raises(B2SError, match="HIP device"):
        vocoder.trim_silence_intervals_batch(torch.zeros(2, 400), [400, 300])
    assert vocoder.trim_params() == R.TRIM_PARAMS


def test_trim_hparam_defaults_to_reference():
    import hyperparams
    hp = fresh_hp()
    assert hp.trim == "reference" and hyperparams.DEFAULTS["trim"] == "reference"
    hp.parse("trim=hip")
    assert hp.trim == "hip"
    fresh_hp()


@pytest.mark.parametrize("over,match", [("trim=hip,vocoder=reference", "trim=hip needs vocoder=hip"), ("trim=librosa", "unknown trim 'librosa'"),
                                        ("trim=librosa,vocoder=hip", "unknown trim 'librosa'")])
def test_save_eval_results_refuses_bad_trim_settings(tmp_path, over, match):
    import synthesize
    fresh_hp(over)
    try:
        with pytest.raises(ValueError, match=match):
            synthesize.save_eval_results(["a"], None, np.zeros((1, 4, 80), np.float32), {"encdec": []}, [3], [4], str(tmp_path),
                                         save_trimmed_wave=True)
    finally:
        fresh_hp()
