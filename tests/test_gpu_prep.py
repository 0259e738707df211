"""The batched GPU corpus preparation (b2s_hip.prep, csrc/vocoder/prep.hip) against the NumPy restatement of the reference's
trim_audios (tests/prep_ref.py) and against np.sort, everything compared exactly.

No utterance of the fixture is left out: tests/test_prep_host.py asserts that no frame of it lies within 1e-3 dB of the threshold of
either split, which is the one place where the fp32 frame energies of the GPU could decide differently from the fp64 restatement.  The
order statistic is an integer count over bit patterns and the scaling a single fp32 multiplication, so nothing else has a tolerance."""
import os

import numpy as np
import pytest
import torch

import audio_ref as A
import prep_ref as P
import silence_ref as S

pytestmark = pytest.mark.gpu

WAV2MEL_GATE = 4e-5           # the wav -> mel tolerance of tests/test_gpu_vocoder.py


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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ the order statistic

def _rows(rng):
    """(signal, intervals) pairs: the data kinds x the sizes at which the kernel changes path (one sample, under / at / over one
    float4 group and one 256-thread sweep, more than one tile is the 320 000 row)."""
    rows = []
    for n in (1, 2, 255, 256, 257, 4097):
        x = rng.standard_normal(n + 9).astype(np.float32)
        rows.append((x, [(4, 4 + n)]))                           # off the 16-byte grid, N = n
    g = rng.standard_normal(5000).astype(np.float32)
    rows.append((np.full(3000, -0.37, np.float32), [(0, 3000)]))                                   # all equal
    lo = np.float32(0.75)
    two = np.where(rng.random(3001) < 0.5, lo, np.nextafter(lo, np.float32(1))).astype(np.float32)
    rows.append((two, [(0, 3001)]))                              # equal down to the lowest mantissa bit: every pass decides
    tiny = rng.choice(np.array([0.0, -0.0, 1e-45, -3e-42, 1.1e-38, -1.2e-38, 1e-30], np.float32), 2500)
    rows.append((tiny.astype(np.float32), [(0, 2500)]))          # zeros, -0.0 and denormals
    ties = np.round(g * 4).astype(np.float32) / 4
    rows.append((ties, [(0, 5000)]))                             # heavy ties around any rank
    rows.append((g, [(3, 700), (700, 700), (701, 1300), (2000, 2001), (4093, 5000)]))   # disjoint intervals, one of them empty
    rows.append((g, [(100, 100)]))                               # nothing covered: 0.0
    return rows


@pytest.mark.parametrize("fraction", [0.0, 0.5, 0.95, 0.9999999])
def test_abs_quantile_equals_the_sorted_sample_bit_for_bit(fraction):
    from b2s_hip import prep
    rows = _rows(np.random.default_rng(5))
    dev, lens = padded([x for x, _ in rows])
    ivs = [iv for _, iv in rows]
    got = prep.abs_quantile_batch(dev, lens, ivs, fraction)
    want = np.array([P.abs_quantile(x, iv, fraction) for x, iv in rows], np.float32)
    if fraction > 0.99:
        for (x, iv), w in zip(rows[:6], want):                   # k = N - 1: the maximum
            assert w == np.abs(x[iv[0][0]:iv[0][1]]).max()
    print("fraction %g: got %s want %s" % (fraction, bits(got), bits(want)))
    np.testing.assert_array_equal(bits(got), bits(want))
    again = prep.abs_quantile_batch(dev, lens, ivs, fraction)
    np.testing.assert_array_equal(bits(again), bits(got))
    for i in (3, 8, 10):                                         # a row alone
        x, iv = rows[i]
        one = prep.abs_quantile_batch(x[None].copy(), [len(x)], [iv], fraction)
        assert bits(one)[0] == bits(got)[i]


def test_abs_quantile_of_a_long_row():
    from b2s_hip import prep
    rng = np.random.default_rng(6)
    x = (rng.standard_normal(320000) * np.exp(rng.standard_normal(320000))).astype(np.float32)
    short = rng.standard_normal(999).astype(np.float32)
    dev, lens = padded([short, x])
    ivs = [[(0, 999)], [(0, 320000)]]
    for fraction in (0.0, 0.5, 0.95, 0.999999):
        got = prep.abs_quantile_batch(dev, lens, ivs, fraction)
        want = np.array([P.abs_quantile(short, ivs[0], fraction), P.abs_quantile(x, ivs[1], fraction)], np.float32)
        np.testing.assert_array_equal(bits(got), bits(want))
    parts = [[(0, 999)], [(5, 16381), (16389, 16390), (16390, 200003), (200003, 200003), (250000, 319999)]]
    got = prep.abs_quantile_batch(dev, lens, parts, 0.95)
    assert bits(got)[1] == bits(P.abs_quantile(x, parts[1], 0.95))


# --------------------------------------------------------------------------------------------------------------- trim_audios_batch

def check_against_restatement(ws, want, got):
    out, out_lens, status, n_removed, v95 = got
    assert out.shape == (len(ws), max(len(w) for w in ws) + 4000) and out.dtype == torch.float32
    out = out.cpu().numpy()
    for b, (st, nr, v, o, _) in enumerate(want):
        assert (status[b], n_removed[b]) == (st, nr), (b, status[b], n_removed[b], st, nr)
        if o is None:
            continue
        assert bits(v95[b:b + 1])[0] == bits(v)[()], (b, v95[b], v)
        assert out_lens[b] == len(o), (b, out_lens[b], len(o))
        assert np.array_equal(bits(out[b, :len(o)]), bits(o)), b
        assert not out[b, len(o):].any(), "samples past out_length must be zero"


@pytest.mark.parametrize("gap_threshold", [12288, 16000])
def test_fixture_batch_matches_the_restatement_exactly(gap_threshold):
    from b2s_hip import prep
    ws = P.fixture_batch()
    dev, lens = padded(ws)
    got = prep.trim_audios_batch(dev, lens, gap_threshold)
    want = P.fixture_results(gap_threshold)
    print("status %s n_removed %s v95 %s out_lengths %s" % (got[2].tolist(), got[3].tolist(), got[4].tolist(), got[1].tolist()))
    check_against_restatement(ws, want, got)
    assert got[1].dtype == got[2].dtype == got[3].dtype == np.int32 and got[4].dtype == np.float32


def test_bit_identical_across_runs_and_independent_of_the_batch():
    from b2s_hip import prep
    named = [(n, w) for n, w in P.fixture_named() if n != "too_long"]          # keeps Lmax, and with it the test, small
    ws = [w for _, w in named]
    want = [r for (n, _), r in zip(P.fixture_named(), P.fixture_results(12288)) if n != "too_long"]
    dev, lens = padded(ws)
    a = prep.trim_audios_batch(dev, lens)
    b = prep.trim_audios_batch(dev, lens)
    assert torch.equal(a[0], b[0])
    for x, y in zip(a[1:], b[1:]):
        np.testing.assert_array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y)
    check_against_restatement(ws, want, a)
    # alone, and in another order next to other neighbours: a non-ok utterance (gap, silent, length) disturbs nobody
    order = list(range(len(ws)))[::-1]
    r = prep.trim_audios_batch(*padded([ws[i] for i in order]))
    check_against_restatement([ws[i] for i in order], [want[i] for i in order], r)
    names = [n for n, _ in named]
    for n in ("front2", "no_padding", "tie_run", "clicks"):
        i = names.index(n)
        one = prep.trim_audios_batch(ws[i][None].copy(), [len(ws[i])])
        check_against_restatement([ws[i]], [want[i]], one)
        if want[i][3] is not None:
            assert torch.equal(one[0][0, :one[1][0]], a[0][i, :a[1][i]])


# ---------------------------------------------------------------------------------------------------------------------- end to end

def _write_pcm16(path, y):
    import wave
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.round(np.clip(y, -1, 1) * 32767).astype("<i2").tobytes())


def test_wavs_to_mels_zip_end_to_end(tmp_path):
    from b2s_hip import corpus, prep
    hp = fresh_hp()
    fx = dict(P.fixture_named())
    picks = ["plain", "front1", "back2", "no_padding", "tie_run", "two_bursts_ok", "gap_both", "too_short", "zeros"]
    cdir = str(tmp_path / "mycorpus")
    os.makedirs(os.path.join(cdir, "wavs"))
    lines, read_back = [], {}
    for i, n in enumerate(picks):
        utt = "%s_%s" % ("spka" if i % 2 else "spkb", n.replace("_", ""))
        path = os.path.join(cdir, "wavs", utt + ".wav")
        if i % 2:
            _write_pcm16(path, fx[n])                            # what the restatement sees is the quantised signal
        else:
            prep.write_wav_float32(path, fx[n])
        read_back[utt] = prep.load_wav(path)
        if i % 2 == 0:
            assert np.array_equal(bits(read_back[utt]), bits(fx[n]))
        lines.append("%s|the text of %s|%s|en-us" % (utt, n, utt.split("_")[0]))
    lines.append("spka_missing|no such file|spka|en-us")
    with open(os.path.join(cdir, "metadata.csv"), "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    want = {utt: P.trim_audio(w, 12288, detail=True) for utt, w in read_back.items()}
    for utt, r in want.items():                                  # the quantised signals keep the precondition of exact comparison
        assert S.frames_in_band(read_back[utt], *P.SPLIT1)[0] == 0
        assert "y2" not in r[4] or S.frames_in_band(r[4]["y2"], *P.SPLIT2)[0] == 0
    try:
        res = prep.trim_audios(cdir)
        ok = sorted(u for u, r in want.items() if r[0] == P.OK)
        assert len(ok) >= 5 and res["n_files"] == len(picks) and res["n_skip"] == len(picks) - len(ok)
        assert (res["n_gap"], res["n_len"], res["n_silent"]) == tuple(sum(r[0] == s for r in want.values()) for s in (P.GAP, P.LENGTH, P.SILENT))
        assert sorted(os.listdir(os.path.join(cdir, "proc_wavs"))) == [u + ".wav" for u in ok]
        for u in ok:
            got = prep.load_wav(os.path.join(cdir, "proc_wavs", u + ".wav"))
            assert np.array_equal(bits(got), bits(want[u][3])), u
        assert sorted(bits(np.array(res["max95v"])).tolist()) == sorted(int(bits(want[u][2])[()]) for u in ok)
        assert prep.trim_audios(cdir) is None                    # proc_wavs exists: the corpus is left alone
        meta = prep.recollect_meta(cdir, min_speaker_samples=2)
        assert meta["n_kept"] == len(ok) and meta["n_missing"] == len(picks) + 1 - len(ok) and meta["n_speakers"] == 2
        assert abs(meta["hours"] * 3600 - sum(len(want[u][3]) for u in ok) / 16000.0) < 1e-6
        assert prep.build_mels(cdir) == len(ok)
        for u in ok:
            mel = np.load(os.path.join(cdir, "mels", u + ".npy"))
            ref = A.get_spectrograms(want[u][3])
            assert mel.dtype == np.float32 and mel.shape == (1 + len(want[u][3]) // 200, 80) == ref.shape
            err = float(np.abs(mel - ref).max())
            assert err <= WAV2MEL_GATE, (u, err)
        packed = str(tmp_path / "packed")
        merged = prep.merge_datasets([cdir], ["en-us"], packed, n_eval=2)
        assert (merged["n_train"], merged["n_eval"]) == (len(ok) - 2, 2)
        rows = corpus.read_metadata(os.path.join(packed, "metadata.eval.txt"))
        assert all(int(r["l"]) == 1 + len(want[r["n"][:-4]][3]) // 200 for r in rows)
        import json
        spk = json.load(open(os.path.join(packed, "spk_id.json")))
        lang = json.load(open(os.path.join(packed, "lang_id.json")))
        hp.parse("max_eval_sample_length=100000")
        feeder = corpus.EvalFeeder(os.path.join(packed, "mels.zip"), os.path.join(packed, "metadata.eval.txt"), hp, spk_to_id=spk,
                                   lang_to_id=lang)
        batches = feeder.fetch_data()
        assert len(batches) >= 1 and sum(len(b["names"]) for b in batches) == 2
        assert batches[0]["mel_targets"].shape[-1] == 80
    finally:
        fresh_hp()


def test_errors_raise_b2s_error():
    from b2s_hip import B2SError, prep
    z = torch.zeros(2, 400, device="cuda")
    with pytest.raises(B2SError, match="HIP device"):
        prep.trim_audios_batch(torch.zeros(2, 400), [400, 300])
    for gap in (0, -1):
        with pytest.raises(B2SError, match="gap_threshold must be > 0"):
            prep.trim_audios_batch(z, [400, 300], gap_threshold=gap)
    with pytest.raises(B2SError, match="gap_threshold must be an integer"):
        prep.trim_audios_batch(z, [400, 300], gap_threshold=12288.0)
    for lens in ([400, 1], [401, 300]):
        with pytest.raises(B2SError, match="2..Lmax"):
            prep.trim_audios_batch(z, lens)
        with pytest.raises(B2SError, match="2..Lmax"):
            prep.abs_quantile_batch(z, lens, [[(0, 10)], [(0, 10)]])
    with pytest.raises(B2SError, match="fraction must be in"):
        prep.abs_quantile_batch(z, [400, 300], [[(0, 10)], [(0, 10)]], 1.0)
    with pytest.raises(B2SError, match="float32"):
        prep.trim_audios_batch(z.double(), [400, 300])
