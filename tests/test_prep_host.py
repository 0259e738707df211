"""CPU-only tests of the corpus preparation's host side: the NumPy restatement of the reference's trim_audios (tests/prep_ref.py) against
cases whose answer follows by hand, the coverage and the near-threshold precondition of the fixture the GPU parity tests use, the RIFF
reader / writer, the b2s_voc_prep_* entry points (declared, exported, bound; argument errors without a GPU) and merge_datasets.

Geometry of the hand-derived cases (tests/test_silence_host.py has the same for one burst): constant-amplitude bursts on an exact-zero
floor, body amplitude A, so the loudest 2048-sample frame has mean square A^2.  Frame f of the first split covers [512 f - 1024,
512 f + 1024) and is non-silent when sum(a_i^2 * overlap_i) / 2048 > 1e-4 * A^2: one sample of the body is enough, a burst at 0.05 A
needs 82 samples of overlap and one at 0.2 A needs 6.  An interval runs from 512 * (first non-silent frame) to 512 * (last + 1)."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import prep_ref as P
import silence_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["b2s_voc_prep_abs_quantile", "b2s_voc_prep_trim", "b2s_voc_prep_ws_bytes"]
A = 0.5


def bursts(L, *spec):
    y = np.zeros(L, np.float32)
    for s, e, a in spec:
        y[s:e] = a
    return y


def test_single_burst_margins_and_the_rank_sample():
    L, s, e = 40000, 8000, 30000
    y = bursts(L, (s, e, A))
    c0, c1 = 7168, 31232                                         # 512 * 14: 512 f + 1024 > 8000; 512 * 61: 512 * 60 - 1024 < 30000
    np.testing.assert_array_equal(S.split(y, *P.SPLIT1), [[c0, c1]])
    status, n_removed, v95, out, d = P.trim_audio(y, detail=True)
    assert (status, n_removed) == (P.OK, 0)
    assert d["n_voiced"] == c1 - c0 and d["k"] == int((c1 - c0) * 0.95)
    assert (c1 - c0) - (e - s) <= d["k"] and v95 == np.float32(A)          # the zeros of the interval's rim all sort below the rank
    scaled = np.float32(A) * np.float32(0.244 / float(np.float32(A)))
    assert np.sort(np.abs(d["y2"]))[d["k"]] == scaled and abs(float(scaled) - 0.244) < 2e-8
    # second trim on the cropped signal: frames of 256 / hop 64, one sample of the burst is enough (256e-4 < 1)
    s2, e2 = s - c0, e - c0
    l, r = ((s2 + 128 - 256) // 64 + 1) * 64, -((-(e2 + 128)) // 64) * 64
    assert (d["l"], d["r"]) == (l, r) == (768, 22976)
    assert len(out) == r - l + 4000 and out.dtype == np.float32
    assert not out[:1600 - l].any() and d["pad_left"] == 1600 - l > 0
    np.testing.assert_array_equal(out[1600 - l:1600 - l + len(d["y2"])], d["y2"])       # y2 from its first sample on, then zeros
    assert not out[1600 - l + len(d["y2"]):].any() and d["pad_right"] == 2400 - (len(d["y2"]) - r) > 0
    assert out[s2 + 1600 - l] == scaled and out[s2 + 1600 - l - 1] == 0


def test_front_spike_under_a_tenth_is_removed_when_far_and_kept_when_near():
    far = bursts(42000, (5400, 6600, 0.05 * A), (12600, 36600, A))                  # 6000 samples of silence before the body
    np.testing.assert_array_equal(S.split(far, *P.SPLIT1), [[4608, 7680], [11776, 37888]])     # gap 4096 >= 4096
    status, n_removed, _, out, d = P.trim_audio(far, detail=True)
    assert (status, n_removed, d["kept"]) == (P.OK, 1, [(11776, 37888)])
    near = bursts(42000, (5400, 6600, 0.05 * A), (9100, 33100, A))                  # 2500 samples before the body
    np.testing.assert_array_equal(S.split(near, *P.SPLIT1)[:, 0], [4608, 8192])     # gap 8192 - 7680 = 512
    status, n_removed, _, _, d = P.trim_audio(near, detail=True)
    assert (status, n_removed, len(d["kept"])) == (P.OK, 0, 2)


def test_spike_under_a_quarter_is_removed_only_if_shorter_than_half_its_gap():
    short = bursts(44000, (5000, 6000, 0.2 * A), (14500, 38500, A))
    iv = S.split(short, *P.SPLIT1)
    np.testing.assert_array_equal(iv[:, 0], [4096, 13824])
    assert iv[0, 1] == 7168 and iv[0, 1] - iv[0, 0] <= (13824 - 7168) // 2
    assert P.trim_audio(short)[:2] == (P.OK, 1)
    long_ = bursts(48000, (5000, 11000, 0.2 * A), (19500, 43500, A))
    iv = S.split(long_, *P.SPLIT1)
    np.testing.assert_array_equal(iv[:2].ravel()[:3], [4096, 12288, 18944])
    assert 18944 - 12288 >= 4096 and 12288 - 4096 > (18944 - 12288) // 2
    assert P.trim_audio(long_)[:2] == (P.OK, 0)


def test_two_trailing_spikes_are_both_removed():
    y = bursts(48000, (4000, 28000, A), (34000, 35200, 0.05 * A), (42000, 43200, 0.05 * A))
    np.testing.assert_array_equal(S.split(y, *P.SPLIT1), [[3072, 29184], [33280, 36352], [41472, 44544]])
    status, n_removed, _, _, d = P.trim_audio(y, detail=True)
    assert (status, n_removed, d["kept"]) == (P.OK, 2, [(3072, 29184)])


@pytest.mark.parametrize("silence,want", [(14000, (P.OK, P.OK)), (16000, (P.GAP, P.OK)), (19000, (P.GAP, P.GAP))])
def test_gap_is_measured_between_intervals_not_between_bursts(silence, want):
    """The 2048-sample frames eat about 2 000 samples of a digital gap: 14 000 -> 11 776, 16 000 -> 13 824, 19 000 -> 16 896."""
    y = bursts(60000, (4000, 20000, A), (20000 + silence, 36000 + silence, A))
    iv = S.split(y, *P.SPLIT1)
    assert iv.shape == (2, 2) and iv[1, 0] - iv[0, 1] == {14000: 11776, 16000: 13824, 19000: 16896}[silence]
    assert (P.trim_audio(y, 12288)[0], P.trim_audio(y, 16000)[0]) == want


@pytest.mark.parametrize("length,out_len", [(9088, 13280), (318080, 322272)])
def test_length_is_refused_on_both_sides(length, out_len):
    """The burst starts and ends on multiples of 64 in the cropped signal: l = start - 64, r = end + 128, out_len = length + 4192."""
    y = bursts(4096 + length + 6000, (4096, 4096 + length, A))
    status, n_removed, v95, out = P.trim_audio(y)
    assert (status, n_removed, len(out)) == (P.LENGTH, 0, out_len) and v95 == np.float32(A)
    ok = bursts(4096 + 12000 + 6000, (4096, 4096 + 12000, A))
    assert P.trim_audio(ok)[0] == P.OK


def test_all_zero_input_is_silent():
    assert P.trim_audio(np.zeros(20000, np.float32))[:3] == (P.SILENT, 0, None)


def test_abs_quantile_is_the_sorted_sample():
    y = np.array([0.5, -0.25, -0.0, 3.0, -2.0, 1.0], np.float32)
    assert P.abs_quantile(y, [(0, 6)], 0.5) == np.float32(1.0)               # sorted 0, .25, .5, 1, 2, 3; k = 3
    assert P.abs_quantile(y, [(0, 2), (2, 2), (4, 6)], 0.0) == np.float32(0.25)
    assert P.abs_quantile(y, [(1, 3)], 0.99) == np.float32(0.25) and P.abs_quantile(y, [(1, 1)], 0.5) == 0


def test_fixture_covers_every_branch():
    names = [n for n, _ in P.fixture_named()]
    res = dict(zip(names, P.fixture_results(12288)))
    res16 = dict(zip(names, P.fixture_results(16000)))
    assert set(r[0] for r in res.values()) == {P.OK, P.GAP, P.LENGTH, P.SILENT}
    assert res["zeros"][0] == res["clicks"][0] == P.SILENT          # ref == 0, and v95 == 0 under a full-scale peak
    assert (res["gap_12288_only"][0], res16["gap_12288_only"][0]) == (P.GAP, P.OK)
    assert res["gap_both"][0] == res16["gap_both"][0] == P.GAP and res["two_bursts_ok"][0] == P.OK
    assert len(res["too_short"][3]) < P.MIN_OUT and len(res["too_long"][3]) > P.MAX_OUT
    # removed from the front and from the back: 0, 1 and >= 2 each (the kept range's position in the split tells which end)
    front, back = {}, {}
    for n, w in P.fixture_named():
        iv = [tuple(r) for r in S.split(w, *P.SPLIT1).tolist()]
        kept = res[n][4]["kept"]
        front[n], back[n] = iv.index(kept[0]), len(iv) - 1 - iv.index(kept[-1])
        assert front[n] + back[n] == res[n][1]
    assert {0, 1, 2} <= set(front.values()) and {0, 1, 2} <= set(back.values()) and max(front.values()) >= 3
    assert (front["both"], back["both"]) == (1, 1) and res["short_02_removed"][1] == 1 and res["long_02_kept"][1] == 0
    assert res["spike_near_kept"][1] == 0 and len(res["spike_near_kept"][4]["kept"]) == 2
    zl = S.split(dict(P.fixture_named())["zero_length_tail"], *P.SPLIT1)
    assert zl[-1, 0] == zl[-1, 1] and res["zero_length_tail"][1] == 1      # a zero-length interval, dropped by the back loop
    # padding on both sides, and on neither
    d = res["plain"][4]
    assert d["pad_left"] > 0 and d["pad_right"] > 0
    d = res["no_padding"][4]
    assert res["no_padding"][0] == P.OK and d["pad_left"] == 0 and d["pad_right"] == 0
    assert d["l"] > 1600 and len(d["y2"]) - d["r"] > 2400
    # k = int(N * 0.95) inside a run of equal values
    d = res["tie_run"][4]
    assert d["sorted"][d["k"] - 100] == d["sorted"][d["k"]] == d["sorted"][d["k"] + 100] == np.float32(0.3)


def test_no_fixture_frame_is_near_the_threshold_of_either_split():
    """Precondition of tests/test_gpu_prep.py's exact comparison: the raw signal at (40, 2048, 512) and the scaled, cropped signal at
    (40, 256, 64) have no frame within silence_ref.BAND_DB of the threshold (100 x what an fp32 frame energy can be off by)."""
    nearest = [99.0, 99.0]
    for (name, w), r in zip(P.fixture_named(), P.fixture_results(16000)):
        n, dist = S.frames_in_band(w, *P.SPLIT1)
        assert n == 0, (name, dist)
        nearest[0] = min(nearest[0], dist)
        if "y2" in r[4]:
            n, dist = S.frames_in_band(r[4]["y2"], *P.SPLIT2)
            assert n == 0, (name, dist)
            nearest[1] = min(nearest[1], dist)
    print("nearest frame: %.4f dB in the first split, %.4f dB in the second" % tuple(nearest))
    assert min(nearest) > 10 * S.BAND_DB


# ----------------------------------------------------------------------------------------------------------------------- WAV I/O

def _write_riff(path, tag, bits, rate, channels, payload, extensible=False):
    align = bits // 8 * channels
    if extensible:
        guid = struct.pack("<H", tag) + b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"
        fmt = struct.pack("<HHIIHH", 0xFFFE, channels, rate, rate * align, align, bits) + struct.pack("<HHI", 22, bits, 4) + guid
    else:
        fmt = struct.pack("<HHIIHH", tag, channels, rate, rate * align, align, bits)
    junk = b"LIST" + struct.pack("<I", 3) + b"abc\x00"                     # an odd-sized chunk in front of the data: padded to even
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + junk + b"data" + struct.pack("<I", len(payload)) + payload
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def test_riff_round_trips_for_the_four_sample_formats(tmp_path):
    from b2s_hip import prep
    rng = np.random.default_rng(0)
    y = np.clip(rng.standard_normal(1001) * 0.3, -1, 1)
    p = str(tmp_path / "a.wav")
    i16 = np.round(y * 32767).astype("<i2")
    _write_riff(p, 1, 16, 16000, 1, i16.tobytes())
    got, rate = prep.read_wav(p)
    assert rate == 16000 and got.dtype == np.float32 and prep.wav_info(p) == (16000, 1, 1001)
    np.testing.assert_array_equal(got, (i16.astype(np.float64) / 32768).astype(np.float32))
    np.testing.assert_array_equal(prep.load_wav(p), got)
    i32 = np.round(y * (2 ** 31 - 1)).astype("<i4")
    _write_riff(p, 1, 32, 16000, 1, i32.tobytes(), extensible=True)
    np.testing.assert_array_equal(prep.read_wav(p)[0], (i32.astype(np.float64) / 2 ** 31).astype(np.float32))
    _write_riff(p, 3, 32, 16000, 1, y.astype("<f4").tobytes())
    np.testing.assert_array_equal(prep.read_wav(p)[0], y.astype(np.float32))
    _write_riff(p, 3, 64, 16000, 1, y.astype("<f8").tobytes())
    np.testing.assert_array_equal(prep.read_wav(p)[0], y.astype(np.float32))
    # the float32 writer: bit-exact round trip, header says IEEE float mono
    w = y.astype(np.float32)
    w[:3] = [-0.0, 1e-42, np.float32(0.1)]
    prep.write_wav_float32(p, w)
    assert prep.wav_info(p) == (16000, 1, 1001)
    assert struct.unpack("<H", open(p, "rb").read()[20:22])[0] == 3
    np.testing.assert_array_equal(prep.load_wav(p).view(np.uint32), w.view(np.uint32))


def test_files_that_need_resampling_or_downmixing_are_refused(tmp_path):
    from b2s_hip import B2SError, prep
    p = str(tmp_path / "a.wav")
    _write_riff(p, 1, 16, 22050, 1, np.zeros(100, "<i2").tobytes())
    with pytest.raises(B2SError, match="22050 Hz.*resampling"):
        prep.load_wav(p)
    _write_riff(p, 1, 16, 16000, 2, np.zeros(200, "<i2").tobytes())
    assert prep.read_wav(p)[0].shape == (100, 2)
    with pytest.raises(B2SError, match="2 channel.*not built"):
        prep.load_wav(p)
    os.makedirs(str(tmp_path / "c" / "wavs"))
    _write_riff(str(tmp_path / "c" / "wavs" / "s_1.wav"), 1, 16, 22050, 1, np.zeros(100, "<i2").tobytes())
    with pytest.raises(B2SError, match="resampling"):
        prep.trim_audios(str(tmp_path / "c"))
    _write_riff(p, 1, 24, 16000, 1, bytes(300))
    with pytest.raises(B2SError, match="unsupported sample format"):
        prep.read_wav(p)
    open(p, "wb").write(b"not a wav file at all")
    with pytest.raises(B2SError, match="not a RIFF"):
        prep.read_wav(p)


# ------------------------------------------------------------------------------------------------------------------------- C ABI

def test_new_symbols_are_declared_bound_and_exported():
    from b2s_hip import prep, vocoder
    l = vocoder.load()
    header = open(os.path.join(ROOT, "include", "b2s_vocoder.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(b2s_voc_[a-z0-9_]+)\s*\(", header))
    assert declared == set(vocoder.EXPORTS)
    nm = shutil.which("nm") or shutil.which("llvm-nm")
    assert nm, "no nm to list the library's dynamic symbols with"
    listed = subprocess.run([nm, "-D", "--defined-only", vocoder.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (b2s_voc_[a-z0-9_]+)\b", listed))
    assert exported == declared, exported ^ declared
    for name in NEW_SYMBOLS:
        assert name in declared and getattr(l, name).argtypes == vocoder._PROTOS[name][1]
    for name in ("trim_audios_batch", "abs_quantile_batch", "trim_audios", "recollect_meta", "build_mels", "merge_datasets", "main"):
        assert callable(getattr(prep, name))
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "`libb2s_vocoder.so`, %d entry points" % len(declared) in readme


def test_prep_argument_errors_come_back_as_messages_without_a_gpu():
    from b2s_hip import prep, vocoder
    l = vocoder.load()
    err = lambda: l.b2s_voc_last_error().decode()
    trim_ws, q_ws = l.b2s_voc_prep_ws_bytes(64, 328000, prep.WS_TRIM), l.b2s_voc_prep_ws_bytes(64, 328000, prep.WS_QUANTILE)
    assert trim_ws > 64 * 328000 * 4 > q_ws >= 64 * 2048 * 4
    assert l.b2s_voc_prep_ws_bytes(0, 1000, 0) == 0 and "B must be > 0" in err()
    assert l.b2s_voc_prep_ws_bytes(2, 1, 0) == 0 and "Lmax must be >= 2" in err()
    assert l.b2s_voc_prep_ws_bytes(2, 2 ** 30, 0) == 0 and "too long" in err()
    assert l.b2s_voc_prep_ws_bytes(2, 1000, 7) == 0 and "unknown workspace kind 7" in err()
    none5 = [None] * 5
    assert l.b2s_voc_prep_trim(None, None, 0, 1000, 12288, *none5, None, 0, None) != 0 and "B must be > 0" in err()
    for gap in (0, -5):
        assert l.b2s_voc_prep_trim(None, None, 2, 1000, gap, *none5, None, 0, None) != 0 and "gap_threshold must be > 0" in err()
    assert l.b2s_voc_prep_trim(None, None, 2, 1000, 12288, *none5, None, 0, None) != 0 and "NULL" in err()
    for frac in (-0.1, 1.0, float("nan")):
        assert l.b2s_voc_prep_abs_quantile(None, None, 2, 1000, None, None, 4, frac, None, None, 0, None) != 0
        assert "fraction must be in [0, 1)" in err()
    assert l.b2s_voc_prep_abs_quantile(None, None, 2, 1000, None, None, 0, 0.5, None, None, 0, None) != 0 and "NI must be > 0" in err()
    assert l.b2s_voc_prep_abs_quantile(None, None, 2, 1000, None, None, 4, 0.5, None, None, 0, None) != 0 and "NULL" in err()


def test_batch_calls_refuse_cpu_tensors():
    import torch
    from b2s_hip import B2SError, prep
    with pytest.raises(B2SError, match="HIP device"):
        prep.trim_audios_batch(torch.zeros(2, 400), [400, 300])
    with pytest.raises(B2SError, match="HIP device"):
        prep.abs_quantile_batch(torch.zeros(2, 400), [400, 300], [[(0, 10)], [(0, 10)]])
    with pytest.raises(B2SError, match="gap_threshold must be an integer"):
        prep.trim_audios_batch(torch.zeros(2, 400), [400, 300], gap_threshold=0.5)


def test_name_rules():
    from b2s_hip import prep
    assert [prep.default_gap_threshold(n) for n in ("pt_br", "caito_es_es", "css10_de", "ljspeech", "pt_br2")] == [16000] * 3 + [12288] * 2
    assert prep.default_min_speaker_samples("google_af_za") == 50 and prep.default_min_speaker_samples("ljspeech") == 100
    assert prep.suffix_language("google_af_za") == "af-za"


# ------------------------------------------------------------------------------------------------------------------ merge_datasets

def _hand_made_corpus(root, name, utts, seed):
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, name, "mels"))
    lines, mels = [], {}
    for i, (utt, frames) in enumerate(utts):
        mels[utt] = rng.standard_normal((frames, 80)).astype(np.float32)
        np.save(os.path.join(root, name, "mels", utt + ".npy"), mels[utt])
        lines.append("%s|text %d of %s|%s|xx" % (utt, i, name, utt.split("_")[0]))
    with open(os.path.join(root, name, "metadata.csv"), "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    return mels


def test_merge_datasets_writes_what_the_feeders_read(tmp_path):
    from b2s_hip import corpus, prep
    root = str(tmp_path)
    a = _hand_made_corpus(root, "alpha", [("spkb_%03d" % i, 20 + i) for i in range(7)] + [("spka_%03d" % i, 40 + i) for i in range(5)], 1)
    b = _hand_made_corpus(root, "beta", [("spkc_%03d" % i, 30 + 2 * i) for i in range(6)], 2)
    g = _hand_made_corpus(root, "gamma", [("spka_9%02d" % i, 11 + i) for i in range(3)], 3)          # second corpus of language en-us
    mels = dict(a, **b, **g)
    dirs = [os.path.join(root, n) for n in ("alpha", "beta", "gamma")]
    packed = str(tmp_path / "packed")
    res = prep.merge_datasets(dirs, ["en-us", "de-de", "en-us"], packed, n_eval=4)
    assert (res["n_train"], res["n_eval"]) == (21 - 8, 8)
    assert open(os.path.join(packed, "lang_id.json")).read() == '{\n "en-us": 0,\n "de-de": 1\n}'
    assert list(res["speakers"].items()) == [("spkb", 0), ("spka", 1), ("spkc", 2)]
    z = corpus.MelZip(os.path.join(packed, "mels.zip"))
    rows = {}
    for part in ("train", "eval"):
        rows[part] = corpus.read_metadata(os.path.join(packed, "metadata.%s.txt" % part))
        for lang in ("en-us", "de-de"):
            names = [r["n"] for r in rows[part] if r["i"] == lang]
            assert names == sorted(names)
        for r in rows[part]:
            mel = z.load(r["n"])
            assert int(r["l"]) == mel.shape[0] and np.array_equal(mel, mels[r["n"][:-4]]) and mel.dtype == np.float32
    z.close()
    assert len(rows["eval"]) == 8 and sorted(r["n"][:-4] for p in rows.values() for r in p) == sorted(mels)
    assert [r["i"] for r in rows["eval"]] == ["en-us"] * 4 + ["de-de"] * 4
    assert not open(os.path.join(packed, "metadata.train.txt")).read().endswith("\n")
    keep = {n: open(os.path.join(packed, n), "rb").read() for n in ("metadata.train.txt", "metadata.eval.txt", "lang_id.json", "spk_id.json")}
    prep.merge_datasets(dirs, {"alpha": "en-us", "beta": "de-de", "gamma": "en-us"}, packed, n_eval=4)
    for n, blob in keep.items():
        assert open(os.path.join(packed, n), "rb").read() == blob, n
    with pytest.raises(prep.B2SError, match="no language given for corpus gamma"):
        prep.merge_datasets(dirs, {"alpha": "en-us", "beta": "de-de"}, packed)
