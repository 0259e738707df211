"""CPU-only tests of the opt-in resampling to 16 kHz (resample="hip"): the length rule, the NumPy restatement of librosa 0.6.0's load /
resampy's 'kaiser_best' (tests/resample_ref.py) pinned by properties whose answer follows by hand or analytically, the down-mix order,
and the interface (the two b2s_voc_resample* entry points declared, exported and bound; argument errors without a GPU).

librosa and resampy are not available to this suite, so the restatement is pinned by what the published algorithm implies, not by the
libraries' output.  The gates of the sine / tone / DC tests are 2 x the figure the restatement gave when they were written (the
figure stands beside each gate); the errors of the down-sampling cases are the algorithm's own: resampy truncates index_step to
int(scale * 512), which detunes the filter's gain by up to 0.3 %, and it interpolates the table linearly."""
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = [8000, 11025, 22050, 24000, 32000, 44100, 48000]
NEW_SYMBOLS = ["b2s_voc_resample", "b2s_voc_resample_ws_bytes"]


# ------------------------------------------------------------------------------------------------------------------ the length rule

LENGTH_TABLE = [(2, 44100, 0, 1), (2, 22050, 1, 2), (3, 48000, 1, 1), (441, 22050, 320, 320), (441, 32000, 220, 221), (1000, 22050, 725, 726)]


def test_length_rule_table():
    from b2s_hip import prep
    for n, sr, n_valid, n_out in LENGTH_TABLE:
        assert R.lengths(n, sr) == (n_valid, n_out) == prep.resample_lengths(n, sr), (n, sr)
    assert prep.resample_lengths(12345, 16000) == (12345, 12345)


@pytest.mark.parametrize("orig_sr", RATES)
def test_length_rule_is_floor_and_ceil_of_the_exact_product(orig_sr):
    """Against exact rational arithmetic for N = 1..3000.  Where N * 16000 / orig_sr is an integer the float product may land on either
    side of it (the rule is the float expression as written, and both sides are the right length there); everywhere else it must be the
    floor and the ceiling."""
    from b2s_hip import prep
    for n in range(1, 3001):
        exact = Fraction(n * 16000, orig_sr)
        got = prep.resample_lengths(n, orig_sr)
        assert got == R.lengths(n, orig_sr)
        fl = exact.numerator // exact.denominator
        if exact.denominator == 1:
            assert got[0] in (fl - 1, fl) and got[1] in (fl, fl + 1) and got[0] <= got[1], (n, got)
        else:
            assert got == (fl, fl + 1), (n, got)
    assert [int(min(1.0, 16000.0 / sr) * 512) for sr in (22050, 44100, 48000, 8000)] == [371, 185, 170, 512]
    assert R.filter_table(orig_sr)[2] == int(min(1.0, 16000.0 / orig_sr) * 512)


# -------------------------------------------------------------------------------------------------------------- the filter table

def test_window_anchor_points():
    win = R.base_window()
    assert win.shape == (32769,) and win.dtype == np.float64
    assert win[0] == R.ROLLOFF
    edge = R.ROLLOFF * np.sinc(64 * R.ROLLOFF) / np.i0(R.BETA)           # the Kaiser taper ends at I0(0) / I0(beta) = 1 / I0(beta)
    assert abs(win[32768] - edge) <= 1e-12 * abs(edge) and abs(edge) < 1e-7
    for m in range(1, 61):                                               # sinc(rolloff * k / 512) changes sign at k = 512 m / rolloff
        k = 512 * m / R.ROLLOFF
        lo, hi = int(np.floor(k)), int(np.ceil(k))
        assert lo != hi and win[lo] * win[hi] < 0, m
        assert np.all(win[int(np.ceil(512 * (m - 1) / R.ROLLOFF)) + 1:lo] * win[lo] > 0)      # and nowhere between two crossings
    # the power series of I0, which is what the kernel sums, against np.i0
    for x in (0.0, 1.0, 7.3, R.BETA):
        q, term, total = 0.25 * x * x, 1.0, 1.0
        for k in range(1, 200):
            term *= q / (k * k)
            total += term
        assert abs(total - np.i0(x)) <= 1e-13 * np.i0(x)
    for sr in (22050, 48000):
        w, d, step, scale, ratio = R.filter_table(sr)
        np.testing.assert_array_equal(w, win * ratio)
        np.testing.assert_array_equal(d[:-1], w[1:] - w[:-1])
        assert d[32768] == 0
    w, d, step, scale, ratio = R.filter_table(8000)
    np.testing.assert_array_equal(w, win)
    assert (step, scale, ratio) == (512, 1.0, 2.0)


def _impulse(n, k):
    x = np.zeros(n, np.float32)
    x[k] = 1.0
    return x


@pytest.mark.parametrize("k", [0, 100, 199])
def test_impulse_response_reads_the_table_at_the_hand_computed_offsets(k):
    """An impulse at input sample k, N = 200.  Three rates whose sample positions are exact in binary, so the offsets follow by hand:
      8000 (ratio 2, step 512): output t sits at input position t / 2.  Even t: position n = t / 2 exactly, offset 0, the weight of
        sample k is win[|n - k| * 512] (left wing i = n - k; right wing frac' = 1, offset 512, tap j = k - n - 1: 512 + 512 j).
        Odd t: n = (t - 1) / 2, frac 0.5, offset 256 on both wings: win[256 + 512 (n - k)] left, win[256 + 512 (k - n - 1)] right.
      32000 (ratio 0.5, step 256, table halved): position 2 t, offset 0 left, 256 right: 0.5 * win[256 |2 t - k|].
      48000 (ratio 1/3, step 170, table / 3): position 3 t, offset 0 left: win[170 (3 t - k)] / 3; right wing frac' = scale,
        idx = 512 / 3 = 170.67, offset 170, eta = 2/3: the linear interpolation between entries 170 j' + 170 and + 171, j' = k - 3 t - 1.
    A tap index past the wing's count (nwin - offset) // step gives no contribution."""
    N = 200
    x = _impulse(N, k)
    base = R.base_window()

    def tab(o, mult=1.0):
        return base[o] * mult if 0 <= o < 32769 else 0.0

    # 8000 Hz
    y = R.resample(x, 8000)
    assert len(y) == 400
    for t in sorted(set(t for t in (2 * k - 20, 2 * k - 7, 2 * k, 2 * k + 1, 2 * k + 30, 0, 399) if 0 <= t < 400)):
        n, odd = t // 2, t % 2
        if k <= n:
            i = n - k
            want = tab(256 * odd + 512 * i) if i < (32769 - 256 * odd) // 512 else 0.0
        else:
            j = k - n - 1
            off = 256 if odd else 512
            want = tab(off + 512 * j) if j < (32769 - off) // 512 else 0.0
        assert y[t] == want, (t, y[t], want)
    assert y[2 * k] == R.ROLLOFF
    # 32000 Hz
    y = R.resample(x, 32000)
    assert len(y) == 100
    for t in sorted(set(t for t in (k // 2 - 9, k // 2, k // 2 + 1, k // 2 + 17, 0, 99) if 0 <= t < 100)):
        d = 2 * t - k
        if d >= 0:
            want = tab(256 * d, 0.5) if d < 32769 // 256 else 0.0
        else:
            want = tab(256 * -d, 0.5) if -d - 1 < (32769 - 256) // 256 else 0.0
        assert y[t] == want, (t, y[t], want)
    # 48000 Hz
    y = R.resample(x, 48000)
    assert len(y) == 67 and R.lengths(N, 48000) == (66, 67) and y[66] == 0
    third = 16000.0 / 48000
    w3 = base * third
    idx = third * 512
    eta = idx - 170
    assert int(idx) == 170
    for t in sorted(set(t for t in (k // 3 - 5, k // 3, k // 3 + 1, k // 3 + 11, 0, 65) if 0 <= t < 66)):
        d = 3 * t - k
        if d >= 0:
            want = w3[170 * d] if d < 32769 // 170 else 0.0
        else:
            j = -d - 1
            o = 170 + 170 * j
            want = w3[o] + eta * (w3[o + 1] - w3[o]) if j < (32769 - 170) // 170 else 0.0
        assert y[t] == want, (t, y[t], want)


def _sine(f, sr, n):
    return np.sin(2 * np.pi * f * np.arange(n) / sr)


def _inner(orig_sr, n):
    """The outputs whose two wings lie inside the signal."""
    step, ratio = R.filter_table(orig_sr)[2], 16000.0 / orig_sr
    e = int(np.ceil((R.NWIN // step + 1) * ratio)) + 1
    return slice(e, R.lengths(n, orig_sr)[0] - e)


# (orig_sr, Hz, gate): max |y - sin| over the inner outputs of 0.25 s, gate = 2 x the figure measured with the restatement (in brackets)
SINE_GATES = [
    (8000, 1000, 7.0e-8),      # [3.452e-08]  up-sampling: the table's own interpolation error
    (8000, 3000, 1.2e-7),      # [5.504e-08]
    (32000, 3000, 6.2e-8),     # [3.069e-08]  ratio 1/2: index_step = 256 exactly, nothing is truncated
    (32000, 7000, 8.0e-7),     # [3.990e-07]
    (22050, 3000, 1.9e-3),     # [9.345e-04]  int(371.52) = 371 detunes the gain
    (22050, 7000, 4.9e-3),     # [2.434e-03]
    (44100, 3000, 6.1e-3),     # [3.047e-03]  int(185.76) = 185
    (44100, 7000, 1.06e-2),    # [5.282e-03]
]


@pytest.mark.parametrize("orig_sr,hz,gate", SINE_GATES)
def test_in_band_sine_comes_out_as_the_analytic_sine(orig_sr, hz, gate):
    n = int(0.25 * orig_sr)
    y = R.resample(_sine(hz, orig_sr, n).astype(np.float32), orig_sr)
    want = _sine(hz, 16000, len(y))
    inner = _inner(orig_sr, n)
    err = float(np.abs(y - want)[inner].max())
    print("%d Hz at %d Hz: max |y - sin| = %.3e (gate %.3e)" % (hz, orig_sr, err, gate))
    assert inner.stop - inner.start > 1000 and err <= gate


# (orig_sr, gate on the 9.5 kHz tone's amplitude [measured], gate on |DC gain - 1| [measured])
STOPBAND_DC_GATES = [(22050, 1.13e-3, 1.14e-3),     # [5.606e-04] [5.691e-04]
                     (44100, 1.11e-3, 5.5e-3)]      # [5.545e-04] [2.741e-03]


@pytest.mark.parametrize("orig_sr,tone_gate,dc_gate", STOPBAND_DC_GATES)
def test_a_tone_above_the_new_nyquist_is_removed_and_dc_keeps_its_level(orig_sr, tone_gate, dc_gate):
    n = int(0.25 * orig_sr)
    inner = _inner(orig_sr, n)
    tone = float(np.abs(R.resample(_sine(9500, orig_sr, n).astype(np.float32), orig_sr))[inner].max())
    dc = float(np.abs(R.resample(np.ones(n, np.float32), orig_sr)[inner] - 1).max())
    print("%d Hz: 9.5 kHz tone comes out at %.3e (gate %.3e), |DC gain - 1| = %.3e (gate %.3e)" % (orig_sr, tone, tone_gate, dc, dc_gate))
    assert tone <= tone_gate and dc <= dc_gate
    assert dc > 1e-4                     # the gain error of the truncated index_step belongs to the algorithm; it is not "fixed" away


def test_fp32_accumulation_mode_and_the_identity_rate():
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, 3000).astype(np.float32)
    a, b = R.resample(x, 22050), R.resample(x, 22050, fp32=True)
    assert a.dtype == np.float64 and b.dtype == np.float32 and a.shape == b.shape == (R.lengths(3000, 22050)[1],)
    assert 0 < float(np.abs(a - b).max()) < 2e-6
    same = R.resample(x, 16000, fp32=True)
    np.testing.assert_array_equal(same.view(np.uint32), x.view(np.uint32))
    y = R.resample(x[:441], 32000)
    assert len(y) == 221 and y[220] == 0 and y[219] != 0            # n_valid = 220 < n_out = 221: the last sample is fix_length's zero
    assert R.resample(x[:2], 44100).tolist() == [0.0]               # n_valid = 0, n_out = 1


# ----------------------------------------------------------------------------------------------------------------------- down-mix

@pytest.mark.parametrize("channels", [2, 3, 6, 8])
def test_sequential_fp32_downmix_is_np_mean_bit_for_bit(channels):
    rng = np.random.default_rng(channels)
    y = (rng.standard_normal((channels, 5001)) * np.exp(rng.standard_normal((channels, 5001)))).astype(np.float32)
    got = R.downmix(y)
    want = np.mean(y, axis=0)
    assert got.dtype == want.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(R.load(y.T.copy(), 16000, fp32=True).view(np.uint32), want.view(np.uint32))
    one = R.downmix(y[:1])
    np.testing.assert_array_equal(one.view(np.uint32), y[0].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------- interface

def test_resample_symbols_are_declared_bound_and_exported():
    from b2s_hip import prep, vocoder
    l = vocoder.load()
    header = open(os.path.join(ROOT, "include", "b2s_vocoder.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(b2s_voc_[a-z0-9_]+)\s*\(", header))
    assert len(declared) == 13 and declared == set(vocoder.EXPORTS)
    nm = shutil.which("nm") or shutil.which("llvm-nm")
    assert nm, "no nm to list the library's dynamic symbols with"
    listed = subprocess.run([nm, "-D", "--defined-only", vocoder.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (b2s_voc_[a-z0-9_]+)\b", listed))
    for name in NEW_SYMBOLS:
        assert name in declared and name in exported and getattr(l, name).argtypes == vocoder._PROTOS[name][1]
    for name in ("resample_batch", "resample_lengths", "resample_tile", "load_wav", "trim_audios"):
        assert callable(getattr(prep, name))
    assert "`libb2s_vocoder.so`, 13 entry points" in open(os.path.join(ROOT, "README.md")).read()


def test_resample_argument_errors_come_back_as_messages_without_a_gpu():
    from b2s_hip import vocoder
    l = vocoder.load()
    err = lambda: l.b2s_voc_last_error().decode()
    table_bytes = 4 * 32769
    mono, stereo = l.b2s_voc_resample_ws_bytes(64, 882000, 1, 44100), l.b2s_voc_resample_ws_bytes(64, 882000, 2, 44100)
    assert table_bytes <= mono < table_bytes + 4096 and stereo == mono + 64 * 882000 * 4
    for B in (0, -3):
        assert l.b2s_voc_resample_ws_bytes(B, 1000, 1, 22050) == 0 and "B must be > 0" in err()
    assert l.b2s_voc_resample_ws_bytes(2, 0, 1, 22050) == 0 and "Lmax_in must be >= 1" in err()
    for c in (0, 9, -1):
        assert l.b2s_voc_resample_ws_bytes(2, 1000, c, 22050) == 0 and "channels must be in 1..8" in err()
    for sr in (3999, 192001, 0, -16000):
        assert l.b2s_voc_resample_ws_bytes(2, 1000, 1, sr) == 0 and "orig_sr must be in 4000..192000" in err()
    assert l.b2s_voc_resample_ws_bytes(2, 1000, 1, 4000) > 0 and l.b2s_voc_resample_ws_bytes(2, 1, 8, 192000) > 0

    def call(B=2, Lmax_in=1000, channels=1, orig_sr=22050, Lmax_out=726, ptrs=(None,) * 6, ws_bytes=0):
        wav, lengths, n_valid, n_out, out, ws = ptrs
        return l.b2s_voc_resample(wav, lengths, B, Lmax_in, channels, orig_sr, n_valid, n_out, Lmax_out, out, ws, ws_bytes, None)

    assert call(B=0) != 0 and "B must be > 0" in err()
    assert call(Lmax_in=0) != 0 and "Lmax_in must be >= 1" in err()
    assert call(channels=9) != 0 and "channels must be in 1..8" in err()
    assert call(orig_sr=3000) != 0 and "orig_sr must be in 4000..192000" in err()
    for bad in (0, -1):
        assert call(Lmax_out=bad) != 0 and "Lmax_out must be >= 1" in err()
    assert call() != 0 and "NULL" in err()
    # every pointer given (host memory: the call must stop at the workspace check, before anything touches them), workspace too small
    import ctypes as C
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    for missing in range(6):
        assert call(ptrs=tuple(None if i == missing else p for i in range(6)), ws_bytes=1 << 30) != 0 and "NULL" in err()
    need = l.b2s_voc_resample_ws_bytes(2, 1000, 2, 22050)
    assert call(channels=2, ptrs=(p,) * 6, ws_bytes=need - 1) != 0
    assert "workspace of %d bytes, %d needed" % (need - 1, need) in err()


def test_resample_batch_refuses_cpu_tensors_and_bad_arguments():
    import torch
    from b2s_hip import B2SError, prep
    with pytest.raises(B2SError, match="HIP device"):
        prep.resample_batch(torch.zeros(2, 400), [400, 300], 22050)
    with pytest.raises(B2SError, match="HIP device"):
        prep.resample_batch(torch.zeros(2, 400, 2), [400, 300], 44100)
    with pytest.raises(B2SError, match="orig_sr must be an integer"):
        prep.resample_batch(torch.zeros(2, 400), [400, 300], 22050.0)
    with pytest.raises(B2SError, match=r"\[B, Lmax\] or \[B, Lmax, C\]"):
        prep.resample_batch(torch.zeros(400), [400], 22050)
    with pytest.raises(B2SError, match="float32"):
        prep.resample_batch(torch.zeros(2, 400, dtype=torch.float64), [400, 300], 22050)


def test_unknown_resample_value_raises_and_the_flag_is_listed(tmp_path, capsys):
    from b2s_hip import prep
    p = str(tmp_path / "a.wav")
    prep.write_wav_float32(p, np.zeros(100, np.float32), sr=22050)
    with pytest.raises(ValueError, match="unknown resample"):
        prep.load_wav(p, resample="bogus")
    os.makedirs(str(tmp_path / "c" / "wavs"))
    with pytest.raises(ValueError, match="unknown resample"):
        prep.trim_audios(str(tmp_path / "c"), resample="librosa")
    assert not os.path.exists(str(tmp_path / "c" / "proc_wavs"))
    with pytest.raises(prep.B2SError, match="22050 Hz.*resampling"):            # the default still refuses, with today's words
        prep.load_wav(p)
    with pytest.raises(SystemExit) as e:
        prep.main(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--resample" in text and "hip" in text
    with pytest.raises(SystemExit):
        prep.main(["--corpus", "x=en", "--packed", "y", "--resample", "cpu"])


def test_tile_rule_restated_in_python():
    """b2s_hip.prep.resample_tile restates make_plan of csrc/vocoder/resample.hip: the largest tile of 4096 / 2^k >= 256 outputs whose
    input span fits 8064 floats of LDS beside the table."""
    from b2s_hip import prep
    assert prep.resample_tile(8000) == (4096, 2048 + 2 * 64 + 4)
    assert prep.resample_tile(22050)[0] == 4096 and prep.resample_tile(44100)[0] == 2048 and prep.resample_tile(48000)[0] == 2048
    assert prep.resample_tile(192000)[0] == 512
    for sr in RATES + [4000, 96000, 192000]:
        tile, span = prep.resample_tile(sr)
        assert span % 4 == 0 and span <= 8064 and 4 * (span + 32832) <= 160 * 1024
