"""The batched GPU down-mix and resampling to 16 kHz (b2s_hip.prep.resample_batch, csrc/vocoder/resample.hip) against the fp64 NumPy
restatement of librosa 0.6.0's load / resampy's 'kaiser_best' (tests/resample_ref.py), and the exact facts of its interface.

The gate.  The kernel's tap loop is fp32 over an fp32 table; resampy itself accumulates into a float32 output.  The restatement has that
mode (fp32=True: fp64 weight times sample, the running sum rounded to fp32 after every tap), and its distance from the fp64 result on the
very rows of this fixture is the yardstick: gate = 4 x max |ref32 - ref64| per sample rate, computed here on the CPU and never from the
GPU's output.  When this file was written that distance was 1.03e-6 to 1.56e-6 depending on the rate (printed by the test), so the
gates are 4.1e-6 to 6.2e-6 on signals of amplitude <= 1; the kernel's own distance was within 4 % of the yardstick at every rate.

Rows.  resample_tile(orig_sr) gives the kernel's two sizes: the outputs a workgroup owns (4096 at 8000 .. 24000 Hz, 2048 at 32000, 44100
and 48000 Hz) and the input samples it stages in LDS.  Every rate gets rows of 2, 3 and 50 samples (shorter than one filter wing), a row
with n_valid < n_out and one with n_valid == n_out, rows whose n_valid is the last value under the tile, the tile itself and the first
value over it (at 8000 Hz n_valid = 2 N is always even and equal to n_out, so `under` and `over` are tile - 2 and tile + 2 there and
the n_valid < n_out row does not exist), and rows of span - 1, span and span + 1 input samples."""
import functools
import os
import struct

import numpy as np
import pytest
import torch

import prep_ref as P
import resample_ref as R
import silence_ref as S

pytestmark = pytest.mark.gpu

RATES = [8000, 11025, 22050, 24000, 32000, 44100, 48000]
GATE_FACTOR = 4.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def padded(ws, fill=0.0):
    pad = np.full((len(ws), max(len(w) for w in ws)) + ws[0].shape[1:], fill, np.float32)
    for i, w in enumerate(ws):
        pad[i, :len(w)] = w
    return pad, [len(w) for w in ws]


def _length_with(orig_sr, pred, start, stop):
    for n in range(start, stop):
        if pred(*R.lengths(n, orig_sr)):
            return n
    return None


def row_lengths(orig_sr):
    """The three groups of input lengths described in the module docstring."""
    from b2s_hip import prep
    tile, span = prep.resample_tile(orig_sr)
    approx = int(tile * orig_sr / 16000.0)
    under = max(n for n in range(approx - 8, approx + 8) if R.lengths(n, orig_sr)[0] < tile)
    at = _length_with(orig_sr, lambda v, o: v == tile, approx - 8, approx + 8)
    over = _length_with(orig_sr, lambda v, o: v > tile, approx - 8, approx + 8)
    assert at is not None and over is not None
    short = [2, 3, 50, _length_with(orig_sr, lambda v, o: v == o, 900, 1400)]
    ragged = _length_with(orig_sr, lambda v, o: v < o, 1000, 1400)
    assert (ragged is None) == (16000 % orig_sr == 0)
    if ragged is not None:
        short.append(ragged)
    return short + [under, at, over], [span - 1, span, span + 1]


@functools.lru_cache(maxsize=None)
def fixture(orig_sr):
    """(batches, gate): every batch a tuple of float32 rows; ref64 of every row; the gate of the rate.  Built once per rate."""
    rng = np.random.default_rng(orig_sr)
    tiles, spans = row_lengths(orig_sr)
    noise = lambda n: rng.uniform(-1.0, 1.0, n).astype(np.float32)

    def impulse(n, k):
        x = np.zeros(n, np.float32)
        x[k] = 1.0
        return x

    t = np.arange(2000)
    batches = [
        [noise(n) for n in tiles],
        [noise(n) for n in spans] + [np.ones(1500, np.float32), np.sin(2 * np.pi * 3000 * t / orig_sr).astype(np.float32),
                                     np.sin(2 * np.pi * 7000 * t / orig_sr).astype(np.float32)],
        [impulse(700, 0), impulse(700, 350), impulse(700, 699)],
    ]
    refs = [[R.resample(w, orig_sr) for w in batch] for batch in batches]
    worst = max(float(np.abs(R.resample(w, orig_sr, fp32=True) - r).max()) for batch, rb in zip(batches, refs) for w, r in zip(batch, rb))
    for batch in batches:
        assert len(batch) <= 8 and max(len(w) for w in batch) <= 40000
        for w in batch:
            w.flags.writeable = False
    return batches, refs, worst


@pytest.mark.parametrize("orig_sr", RATES)
def test_parity_with_the_fp64_restatement(orig_sr):
    from b2s_hip import prep
    batches, refs, worst = fixture(orig_sr)
    gate = GATE_FACTOR * worst
    assert 1e-7 < worst < 2e-6                       # the yardstick itself: fp32 accumulation over a few hundred taps of amplitude <= 1
    seen = 0.0
    for batch, rb in zip(batches, refs):
        pad, lens = padded(batch)
        out, out_lens = prep.resample_batch(torch.from_numpy(pad).cuda(), lens, orig_sr)
        assert out.dtype == torch.float32 and out.is_cuda and out_lens.dtype == np.int32
        assert out.shape == (len(batch), max(1, max(len(r) for r in rb)))
        got = out.cpu().numpy()
        for b, (w, r) in enumerate(zip(batch, rb)):
            n_valid, n_out = R.lengths(len(w), orig_sr)
            assert out_lens[b] == n_out == len(r)
            err = float(np.abs(got[b, :n_out] - r).max())
            seen = max(seen, err)
            assert err <= gate, (orig_sr, len(w), err, gate)
            assert not bits(got[b, n_valid:]).any(), "samples from n_valid on must be exactly 0.0"
    print("%d Hz: max |gpu - ref64| = %.3e, max |ref32 - ref64| = %.3e, gate %.3e" % (orig_sr, seen, worst, gate))


def test_rate_16000_returns_the_input_bits():
    from b2s_hip import prep
    rng = np.random.default_rng(1)
    ws = [rng.standard_normal(n).astype(np.float32) for n in (1, 2, 255, 257, 5000)]
    ws[3][:4] = [-0.0, 1e-42, -3e-39, np.float32(0.1)]
    pad, lens = padded(ws, fill=np.nan)
    out, out_lens = prep.resample_batch(pad, lens, 16000)
    got = out.cpu().numpy()
    assert out_lens.tolist() == lens and got.shape == pad.shape
    for b, w in enumerate(ws):
        np.testing.assert_array_equal(bits(got[b, :len(w)]), bits(w))
        assert not bits(got[b, len(w):]).any()


@pytest.mark.parametrize("orig_sr", [22050, 44100, 8000])
def test_padding_repeat_and_batch_independence(orig_sr):
    """NaN in the padding past `lengths` never reaches the output; a second call gives the same bits; a row alone equals the row in the
    batch."""
    from b2s_hip import prep
    batch = fixture(orig_sr)[0][0]
    clean, lens = padded(batch)
    dirty, _ = padded(batch, fill=np.nan)
    a, out_lens = prep.resample_batch(clean, lens, orig_sr)
    b, _ = prep.resample_batch(dirty, lens, orig_sr)
    c, _ = prep.resample_batch(dirty, lens, orig_sr)
    assert not torch.isnan(b).any()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(b.view(torch.int32), c.view(torch.int32))
    a = a.cpu().numpy()
    for i in (0, 2, len(batch) - 2, len(batch) - 1):
        one, n = prep.resample_batch(batch[i][None].copy(), [len(batch[i])], orig_sr)
        assert n[0] == out_lens[i]
        np.testing.assert_array_equal(bits(one.cpu().numpy()[0, :n[0]]), bits(a[i, :n[0]]))


@pytest.mark.parametrize("channels", [2, 3, 6, 8])
def test_downmix_equals_np_mean_bit_for_bit(channels):
    from b2s_hip import prep
    rng = np.random.default_rng(channels)
    ws = [(rng.standard_normal((n, channels)) * np.exp(rng.standard_normal((n, channels)))).astype(np.float32) for n in (1, 300, 4099)]
    pad, lens = padded(ws, fill=np.nan)
    out, out_lens = prep.resample_batch(pad, lens, 16000)
    got = out.cpu().numpy()
    for b, w in enumerate(ws):
        want = np.mean(np.ascontiguousarray(w.T), axis=0)        # float32 [C, N] in memory: NumPy adds the rows one after another
        np.testing.assert_array_equal(bits(got[b, :len(w)]), bits(want))
        np.testing.assert_array_equal(bits(want), bits(R.downmix(w.T)))
        assert not bits(got[b, len(w):]).any()


def test_stereo_44100_equals_the_mono_path_on_its_mean():
    from b2s_hip import prep
    rng = np.random.default_rng(9)
    ws = [rng.uniform(-1, 1, (n, 2)).astype(np.float32) for n in (3000, 5700)]
    pad, lens = padded(ws, fill=np.nan)
    stereo, n1 = prep.resample_batch(pad, lens, 44100)
    mono_pad, _ = padded([np.mean(w.T, axis=0) for w in ws])
    mono, n2 = prep.resample_batch(mono_pad, lens, 44100)
    assert n1.tolist() == n2.tolist() and torch.equal(stereo.view(torch.int32), mono.view(torch.int32))
    ref = R.load(ws[1], 44100)
    assert float(np.abs(stereo.cpu().numpy()[1, :len(ref)] - ref).max()) <= GATE_FACTOR * float(np.abs(R.load(ws[1], 44100, fp32=True) - ref).max())


def test_errors_raise_b2s_error():
    from b2s_hip import B2SError, prep
    z = torch.zeros(2, 400, device="cuda")
    with pytest.raises(B2SError, match="HIP device"):
        prep.resample_batch(z.cpu(), [400, 300], 22050)
    with pytest.raises(B2SError, match="channels must be in 1..8"):
        prep.resample_batch(torch.zeros(2, 40, 9, device="cuda"), [40, 30], 22050)
    for sr in (3999, 192001):
        with pytest.raises(B2SError, match="orig_sr must be in 4000..192000"):
            prep.resample_batch(z, [400, 300], sr)
    for lens in ([400, 0], [401, 300]):
        with pytest.raises(B2SError, match="1..Lmax"):
            prep.resample_batch(z, lens, 22050)
    with pytest.raises(B2SError, match="lengths for a batch"):
        prep.resample_batch(z, [400], 22050)


# ---------------------------------------------------------------------------------------------------------------------- end to end

def _write_riff(path, tag, bits_, rate, channels, payload):
    align = bits_ // 8 * channels
    fmt = struct.pack("<HHIIHH", tag, channels, rate, rate * align, align, bits_)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(payload)) + payload
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def test_trim_audios_resamples_a_mixed_corpus(tmp_path):
    """proc_wavs/ must be the restatement of trim_audios (tests/prep_ref.py) applied to the GPU-resampled signal: the resampling stage is
    checked by the tests above, the trimming by tests/test_gpu_prep.py, and this one that the two are joined without a change."""
    from b2s_hip import B2SError, prep
    cdir = str(tmp_path / "mixed")
    os.makedirs(os.path.join(cdir, "wavs"))
    path = lambda n: os.path.join(cdir, "wavs", n + ".wav")
    a = P._compose(21, 26000, [(3000, 20000, 0.6)])
    _write_riff(path("spka_pcm22k"), 1, 16, 22050, 1, np.round(np.clip(a, -1, 1) * 32767).astype("<i2").tobytes())
    left = P._compose(22, 44100, [(6000, 36000, 0.6)])
    stereo = np.stack([left, (0.5 * left + P._compose(23, 44100, [])).astype(np.float32)], axis=1)
    _write_riff(path("spka_f32stereo44k"), 3, 32, 44100, 2, stereo.astype("<f4").tobytes())
    c = dict(P.fixture_named())["plain"]
    prep.write_wav_float32(path("spkb_plain16k"), c)
    _write_riff(path("spkb_tiny"), 1, 16, 44100, 1, np.zeros(2, "<i2").tobytes())          # n_valid 0, n_out 1: skipped for length
    with pytest.raises(B2SError, match="resampling"):                                       # today's behaviour, today's message
        prep.trim_audios(cdir)
    assert not os.path.exists(os.path.join(cdir, "proc_wavs"))
    with pytest.raises(B2SError, match="22050 Hz.*resampling"):
        prep.load_wav(path("spka_pcm22k"))

    loaded = {n: prep.load_wav(path(n), resample="hip") for n in ("spka_pcm22k", "spka_f32stereo44k", "spkb_plain16k", "spkb_tiny")}
    assert [len(loaded[n]) for n in ("spka_pcm22k", "spka_f32stereo44k", "spkb_plain16k", "spkb_tiny")] == \
        [R.lengths(26000, 22050)[1], R.lengths(44100, 44100)[1], len(c), 1]
    assert all(v.dtype == np.float32 and v.ndim == 1 for v in loaded.values())
    np.testing.assert_array_equal(bits(loaded["spkb_plain16k"]), bits(c))
    read = prep.read_wav(path("spka_pcm22k"))[0]
    ref = R.load(read, 22050)
    assert float(np.abs(loaded["spka_pcm22k"] - ref).max()) <= GATE_FACTOR * float(np.abs(R.load(read, 22050, fp32=True) - ref).max())
    ref = R.load(prep.read_wav(path("spka_f32stereo44k"))[0], 44100)
    assert float(np.abs(loaded["spka_f32stereo44k"] - ref).max()) <= GATE_FACTOR * \
        float(np.abs(R.load(stereo, 44100, fp32=True) - ref).max())

    want = {n: P.trim_audio(w, 12288, detail=True) for n, w in loaded.items() if len(w) >= 2}
    for n, r in want.items():                                   # the precondition of an exact comparison (tests/test_prep_host.py)
        assert r[0] == P.OK, (n, r[0])
        assert S.frames_in_band(loaded[n], *P.SPLIT1)[0] == 0 and S.frames_in_band(r[4]["y2"], *P.SPLIT2)[0] == 0
    res = prep.trim_audios(cdir, resample="hip")
    assert res["n_files"] == 4 and res["n_skip"] == 1 == res["n_len"] and res["n_gap"] == res["n_silent"] == 0
    assert res["n_skip"] == res["n_gap"] + res["n_len"] + res["n_silent"] and len(res["max95v"]) == res["n_files"] - res["n_skip"]
    assert sorted(os.listdir(os.path.join(cdir, "proc_wavs"))) == sorted(n + ".wav" for n in want)
    for n, r in want.items():
        out_path = os.path.join(cdir, "proc_wavs", n + ".wav")
        assert prep.wav_info(out_path)[:2] == (16000, 1)
        got = prep.load_wav(out_path)
        assert np.array_equal(bits(got), bits(r[3])), n
    assert sorted(bits(np.array(res["max95v"])).tolist()) == sorted(int(bits(r[2]).reshape(-1)[0]) for r in want.values())
    assert prep.trim_audios(cdir, resample="hip") is None
