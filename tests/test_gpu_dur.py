"""GPU tests of the monotonic alignment search and the duration error (b2s_hip.durations, libb2s_dur.so) against the NumPy
restatement tests/dur_ref.py.

One padded batch [12, 256, 1000] whose (S, T) pairs sit on the wave edges (64 / 65, 128 / 129), on the tight case T == S and on
both sides of the 16-byte load and of the 16-frame block; five contents rotated over the pairs in two assignments; NaN past every
length and sentinels behind every output.  Gates: path, durations and status EQUAL, the score bit-equal (compared as int64).  Every
cell of the search is one fp64 add and one compare in a fixed order, so there is no tolerance to derive: anything but equality is a
defect.  The counts of the error are integers and EQUAL as well."""
import json
import zipfile

import numpy as np
import pytest
import torch

import align_ref
import dur_ref as R

pytestmark = pytest.mark.gpu

PAIRS = [(1, 1), (1, 9), (2, 2), (2, 3), (7, 7), (64, 64), (63, 200), (64, 257), (65, 257), (128, 515), (129, 515), (256, 1000)]
SMAX, TMAX = 256, 1000
CONTENTS = ["staircase", "uniform", "diffuse", "backjump", "zero_columns"]
SHIFT = [0, 2]                               # pair i holds content (i + SHIFT[variant]) % 5


def make_map(kind, S, T, rng):
    """[S, T] fp32, non-negative."""
    if kind == "uniform":
        return np.full((S, T), np.float32(1.0 / S), np.float32)
    if kind == "diffuse":                    # random columns normalised to 1
        p = rng.random((S, T)) + 1e-3
        return (p / p.sum(axis=0, keepdims=True)).astype(np.float32)
    p = R.staircase(rng, R.random_durations(rng, S, T), noise=0.2)
    if kind == "backjump":                   # every fifth frame's maximum sits far from the staircase, before it or after it
        for t in range(2, T, 5):
            p[(int(p[:, t].argmax()) + S // 2 + t) % S, t] = np.float32(1.7)
    if kind == "zero_columns":               # whole frames without any weight, the first and the last among them
        p[:, ::3] = 0.0
        p[:, T - 1] = 0.0
    return p


_cache = {}


def batch(variant):
    """The padded maps (NaN past either length), the lengths and the oracle's results, computed once and left unchanged."""
    if variant not in _cache:
        rng = np.random.default_rng(20260301 + variant)
        maps = np.full((len(PAIRS), SMAX, TMAX), np.nan, np.float32)
        kinds = []
        for i, (S, T) in enumerate(PAIRS):
            kinds.append(CONTENTS[(i + SHIFT[variant]) % len(CONTENTS)])
            maps[i, :S, :T] = make_map(kinds[-1], S, T, rng)
        enc, dec = [p[0] for p in PAIRS], [p[1] for p in PAIRS]
        _cache[variant] = (maps, enc, dec, kinds, R.mas_batch(maps, enc, dec))
    return _cache[variant]


def run_mas(maps, enc, dec, guard=2):
    """b2s_dur_mas through the C ABI with every output pre-filled with a sentinel and `guard` sentinel rows behind it; those must stay
    untouched.  Returns host arrays."""
    from b2s_hip import durations
    l = durations.load()
    dev = torch.device("cuda")
    m = torch.from_numpy(np.ascontiguousarray(maps)).to(dev)
    B, S, T = (int(v) for v in m.shape)
    path = torch.full((B + guard, T), -7, dtype=torch.int32, device=dev)
    dur = torch.full((B + guard, S), -7, dtype=torch.int32, device=dev)
    score = torch.full((B + guard,), -12345.0, dtype=torch.float64, device=dev)
    status = torch.full((B + guard,), -7, dtype=torch.int32, device=dev)
    nbytes = l.b2s_dur_ws_bytes(B, S, T)
    ws = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=dev)
    e, d = (torch.tensor(v, dtype=torch.int32, device=dev) for v in (enc, dec))
    durations.check(l.b2s_dur_mas(m.data_ptr(), e.data_ptr(), d.data_ptr(), B, S, T, path.data_ptr(), dur.data_ptr(), score.data_ptr(),
                                  status.data_ptr(), ws.data_ptr(), nbytes, None))
    torch.cuda.synchronize()
    out = {"path": path.cpu().numpy(), "durations": dur.cpu().numpy(), "score": score.cpu().numpy(), "status": status.cpu().numpy()}
    assert np.all(out["path"][B:] == -7) and np.all(out["durations"][B:] == -7) and np.all(out["status"][B:] == -7)
    assert np.all(out["score"][B:] == -12345.0) and np.all(ws[nbytes:].cpu().numpy() == 0xA5)
    return {k: v[:B] for k, v in out.items()}


def same(got, want):
    """EQUAL path, durations and status, bit-equal score (NaN equal to NaN)."""
    assert np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    assert np.array_equal(got["path"], want["path"])
    assert np.array_equal(got["durations"], want["durations"])
    ok = want["status"] != R.FAILED
    assert np.array_equal(got["score"][ok & ~np.isnan(want["score"])].view(np.int64),
                          want["score"][ok & ~np.isnan(want["score"])].view(np.int64))
    assert np.array_equal(np.isnan(got["score"]), np.isnan(want["score"]))


@pytest.mark.parametrize("variant", [0, 1])
def test_padded_batch_equals_the_oracle(variant):
    maps, enc, dec, kinds, want = batch(variant)
    assert np.all(want["status"] == R.OK) and set(kinds) == set(CONTENTS)
    got = run_mas(maps, enc, dec)
    same(got, want)
    for i, (S, T) in enumerate(PAIRS):
        d, p = got["durations"][i], got["path"][i]
        assert d[:S].sum() == T and d[:S].min() >= 1 and not d[S:].any() and np.all(p[T:] == -1)
        assert p[0] == 0 and p[T - 1] == S - 1 and set(np.diff(p[:T]).tolist()) <= {0, 1}
        if kinds[i] == "uniform":
            assert d[:S].tolist() == [1] * (S - 1) + [T - S + 1]
        if kinds[i] == "backjump" and S >= 7 and T > S:                    # the argmax path is no duration: the search's is
            step = np.diff(maps[i, :S, :T].argmax(axis=0))
            assert step.min() < 0 and step.max() > 1


def test_statuses_leave_the_neighbours_alone():
    rng = np.random.default_rng(3)
    S, T = 8, 10
    maps = rng.random((9, S, T)).astype(np.float32)
    enc = [8, 8, 0, 5, 9, 8, 6, 6, 8]
    dec = [10, 0, 10, 4, 10, 11, 9, 9, 10]
    maps[6, 2, 3] = np.nan                                                 # inside the valid cells
    maps[7, 5, 8] = np.inf
    maps[8, :, :] = rng.random((S, T)).astype(np.float32)
    maps[0, 7, 9] = -0.0
    maps[6, 6:, :] = np.nan                                                # past the lengths: ignored
    maps[7, :, 9:] = np.nan
    want = R.mas_batch(maps, enc, dec)
    assert want["status"].tolist() == [R.OK, R.EMPTY, R.EMPTY, R.SHORT, R.FAILED, R.FAILED, R.FAILED, R.FAILED, R.OK]
    got = run_mas(maps, enc, dec)
    same(got, want)
    for b in range(1, 8):
        assert np.all(got["path"][b] == -1) and not got["durations"][b].any()
    assert got["score"][1] == 0.0 and got["score"][2] == 0.0 and np.isnan(got["score"][3:8]).all()
    clean = maps.copy()
    clean[6, 2, 3], clean[7, 5, 8] = 0.5, 0.5                              # without the two values both are searched
    again = run_mas(clean, enc, dec)
    assert again["status"][6] == again["status"][7] == R.OK
    same(again, R.mas_batch(clean, enc, dec))


def test_a_tiny_first_weight_keeps_its_sign_bit():
    """Tb == 1: the score is p[0][0] itself, a negative zero included."""
    maps = np.array([[[-0.0]], [[0.0]], [[3.5]]], np.float32)
    got = run_mas(maps, [1, 1, 1], [1, 1, 1])
    assert got["score"].view(np.int64).tolist() == np.array([-0.0, 0.0, 3.5]).view(np.int64).tolist()
    assert got["durations"].tolist() == [[1], [1], [1]] and got["path"].tolist() == [[0], [0], [0]]


def test_one_utterance_at_the_limit():
    from b2s_hip import durations
    S, T = durations.MAX_S, 1100
    rng = np.random.default_rng(11)
    d = R.random_durations(rng, S, T)
    maps = R.staircase(rng, d)[None]
    got = run_mas(maps, [S], [T])
    same(got, R.mas_batch(maps, [S], [T]))
    assert got["durations"][0].tolist() == d.tolist()


def test_alone_or_in_the_batch_and_from_run_to_run():
    maps, enc, dec, _, _ = batch(0)
    a, b = run_mas(maps, enc, dec), run_mas(maps, enc, dec)
    for k in a:
        assert np.array_equal(a[k].view(np.int64 if k == "score" else a[k].dtype), b[k].view(np.int64 if k == "score" else b[k].dtype))
    for i, (S, T) in enumerate(PAIRS):                                     # cropped: another T, so other loads and other blocks
        one = run_mas(maps[i:i + 1, :S, :T], [S], [T])
        assert np.array_equal(one["path"][0], a["path"][i, :T]) and np.array_equal(one["durations"][0], a["durations"][i, :S])
        assert one["score"].view(np.int64)[0] == a["score"].view(np.int64)[i] and one["status"][0] == R.OK


def test_python_surface_returns_device_tensors():
    from b2s_hip import durations
    maps, enc, dec, _, want = batch(1)
    out = durations.mas_batch(maps, enc, torch.tensor(dec))
    assert all(out[k].is_cuda for k in ("path", "durations", "score", "status", "mono_focus"))
    same({k: out[k].cpu().numpy() for k in ("path", "durations", "score", "status")}, want)
    assert np.array_equal(out["mono_focus"].cpu().numpy(), want["score"] / np.maximum(np.array(dec), 1))
    empty = durations.mas_batch(np.zeros((0, 4, 5), np.float32), [], [])
    assert empty["path"].shape == (0, 5) and empty["durations"].shape == (0, 4)
    with pytest.raises(durations.B2SError, match="S must be in 1..1024"):
        durations.mas_batch(np.zeros((1, 1025, 4), np.float32), [4], [4])


# ---------------------------------------------------------------------------------------------------------------------- the error

def test_duration_error_counts_equal_the_oracle():
    from b2s_hip import durations
    _, enc, dec, _, ref = batch(0)
    x = ref["durations"].astype(np.int32)
    y = x.copy()
    for i, S in enumerate(enc):
        y[i, :S] = np.roll(x[i, :S], 1)                                    # a shifted copy: the same frames, other positions
    rng = np.random.default_rng(5)
    groups = np.zeros_like(x)
    for i, S in enumerate(enc):
        groups[i, :S] = np.cumsum(rng.random(S) < 0.6) if i % 3 else 0     # every third utterance is one unit over its length
        groups[i, :S] -= groups[i, 0]
        groups[i, S:] = -5
    for g in (None, groups):
        want_c, want_s = R.counts_batch(x, y, enc, g)
        assert np.all(want_s == R.OK)
        out = durations.duration_error_batch(torch.from_numpy(x).cuda(), y, enc, groups=g, frame_ms=12.5)
        assert np.array_equal(out["counts"].cpu().numpy(), want_c) and np.array_equal(out["status"].cpu().numpy(), want_s)
        want = durations.scores_from_counts(want_c, 12.5)
        for k in durations.SCORES:
            assert np.array_equal(out[k].view(np.int64), want[k].view(np.int64))
        assert np.all(want_c[:, 1] == np.array(dec)) and np.all(want_c[:, 2] == np.array(dec))
    same_side = durations.duration_error_batch(x, x, enc)                   # frame_ms from the hyper-parameters
    assert np.all(same_side["rmse_ms"] == 0.0) and np.all(same_side["rate_ratio"] == 1.0)
    # statuses: rows that fail or are empty beside rows that are fine
    S = 6
    dx = np.array([[1, 2, 3, 4, 5, 6]] * 9, np.int32)
    dy = np.array([[2, 2, 2, 4, 0, 9]] * 9, np.int32)
    n = [6, 0, 7, -1, 6, 6, 6, 6, 5]
    g = np.array([[0, 0, 1, 2, 2, 3]] * 9, np.int32)
    dx[4, 3] = -1                                                          # a negative duration
    g[5] = [0, 1, 0, 1, 2, 3]                                              # decreases
    g[6] = [1, 1, 2, 3, 4, 5]                                              # starts above 0
    g[7] = [0, 2, 2, 3, 4, 5]                                              # skips a value
    g[8] = [0, 1, 1, 1, 2, -9]                                             # the bad value is past the length
    want_c, want_s = R.counts_batch(dx, dy, n, g)
    assert want_s.tolist() == [R.OK, R.EMPTY, R.FAILED, R.FAILED, R.FAILED, R.FAILED, R.FAILED, R.FAILED, R.OK]
    out = durations.duration_error_batch(dx, dy, n, groups=g, frame_ms=10.0)
    assert np.array_equal(out["counts"].cpu().numpy(), want_c) and np.array_equal(out["status"].cpu().numpy(), want_s)
    assert want_c[0].tolist() == [4, 21, 19, 1 + 1 + 5 + 3, 1 + 1 + 25 + 9, 9 + 9 + 81 + 36, 16 + 4 + 16 + 81, 12 + 6 + 36 + 54, 9, 9, 0, 0]
    assert np.isnan(out["rmse_frames"][1:8]).all() and out["mae_frames"][0] == 2.5
    big = np.array([[2 ** 31 - 1, 1], [2 ** 31 - 2, 1]], np.int64).astype(np.int32)
    want_c, want_s = R.counts_batch(big, big, [2, 2])
    out = durations.duration_error_batch(big, big, [2, 2], frame_ms=1.0)
    assert want_s.tolist() == [R.FAILED, R.OK] and np.array_equal(out["status"].cpu().numpy(), want_s)
    assert np.array_equal(out["counts"].cpu().numpy(), want_c) and want_c[1, 5] == (2 ** 31 - 2) ** 2 + 1


# ------------------------------------------------------------------------------------------------------------------- from maps

def test_byte_durations_pick_the_head_the_reference_would_plot():
    from b2s_hip import durations
    B, L, H, S, T = 3, 2, 2, 70, 131                                       # two waves, T odd: the dword loads
    enc, dec = [70, 33, 5], [131, 64, 9]
    layers = align_ref.make_case(align_ref.SEED, B, L, H, S, T, enc, dec)  # 7.0 past either length
    sel = align_ref.select(layers, enc, dec)
    want = R.mas_batch(sel["maps"], enc, dec)
    assert np.all(want["status"] == R.OK) and sel["best"].max() > 0
    out = durations.byte_durations(layers, enc, dec)
    assert np.array_equal(out["layer"].cpu().numpy() * H + out["head"].cpu().numpy(), sel["best"])
    same({k: out[k].cpu().numpy() for k in ("path", "durations", "score", "status")}, want)
    focus = out["focus"].cpu().numpy()
    assert np.all(out["mono_focus"].cpu().numpy() <= focus + 1e-12) and np.all(focus <= 1.0 + 1e-6)
    one = torch.from_numpy(sel["maps"][:, None])                           # the [B, 1, S, T] form of hp.align == "hip"
    for form in (one, [one.numpy()], [one.cuda()]):
        again = durations.byte_durations(form, enc, dec)
        same({k: again[k].cpu().numpy() for k in ("path", "durations", "score", "status")}, want)
        assert not again["layer"].cpu().numpy().any() and not again["head"].cpu().numpy().any()
        assert np.array_equal(again["focus"].cpu().numpy().view(np.int64), focus.view(np.int64))


# ------------------------------------------------------------------------------------------------------------------ end to end

@pytest.fixture
def tiny():
    """The tiny fp32 model of smoke() and its batch (B=3, S=11, T=23)."""
    import hyperparams
    from hyperparams import hparams as hp
    from oracle import synth, make_config, TINY96
    from transformer.tacotron import Tacotron
    hp.override_from_dict(hyperparams.DEFAULTS)
    hp.parse(TINY96)
    hp.parse("compute_dtype=fp32,max_generation_frames=40")
    try:
        cfg = make_config(TINY96)
        st = synth.synthetic_state(cfg, 1234)
        m = Tacotron(hp)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in st.items()})
        m = m.to("cuda:0").train()
        nb = synth.synthetic_batch(cfg, B=3, S=11, T=23, seed=7, in_lens=[11, 7, 4], tgt_lens=[23, 15, 9])
        yield m, nb, hp
    finally:
        hp.override_from_dict(hyperparams.DEFAULTS)


def capture_maps(monkeypatch):
    """Wrap durations.byte_durations so that the maps it is handed are kept (host copies, one list per call)."""
    from b2s_hip import durations
    seen, inner = [], durations.byte_durations

    def wrapped(encdec, input_lengths, dec_lengths):
        layers = [encdec] if isinstance(encdec, (torch.Tensor, np.ndarray)) else list(encdec)
        seen.append([(a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)) for a in layers])
        return inner(encdec, input_lengths, dec_lengths)
    monkeypatch.setattr(durations, "byte_durations", wrapped)
    return seen


def test_teacher_forced_durations_on_the_tiny_model(tiny, monkeypatch):
    from b2s_hip import durations
    m, nb, _ = tiny
    seen = capture_maps(monkeypatch)
    out = durations.teacher_forced_durations(m, nb)
    assert m.training and len(seen) == 1                                   # the flag is put back
    layers = seen[0]
    assert len(layers) == 2 and layers[0].shape == (3, 2, 11, 23)
    sel = align_ref.select(layers, nb["input_lengths"], nb["target_lengths"])
    want = R.mas_batch(sel["maps"], nb["input_lengths"], nb["target_lengths"])
    assert np.all(want["status"] == R.OK)
    same({k: out[k].cpu().numpy() for k in ("path", "durations", "score", "status")}, want)
    assert np.array_equal(out["layer"].cpu().numpy() * 2 + out["head"].cpu().numpy(), sel["best"])
    assert out["durations"].cpu().numpy().sum(axis=1).tolist() == [23, 15, 9]
    as_tensors = {k: (torch.from_numpy(np.asarray(v)).cuda() if not isinstance(v, list) else v) for k, v in nb.items()}
    again = durations.teacher_forced_durations(m.eval(), as_tensors)
    assert not m.training and torch.equal(again["durations"], out["durations"])


def test_eval_durations_on_the_tiny_model(tiny, monkeypatch):
    import synthesize
    from b2s_hip import durations
    m, nb, hp = tiny
    m.eval()
    data = {k: (torch.from_numpy(np.asarray(v)).to("cuda:0") if not isinstance(v, list) else v) for k, v in nb.items()}
    data["names"] = ["utt%d" % i for i in range(3)]
    got = {}
    for align in ("reference", "hip"):
        hp.parse("align=%s" % align)
        res = synthesize.eval_batch(m, data, use_bar=False, bar_interval=-1, device_results=(align == "hip"))
        seen = capture_maps(monkeypatch)
        out = durations.eval_durations(m, data, res)
        monkeypatch.undo()
        n_gen = [int(v) for v in _host(res["generated_lengths"])]
        sel = align_ref.select(seen[0], nb["input_lengths"], n_gen)
        want = R.mas_batch(sel["maps"], nb["input_lengths"], n_gen)
        same({k: out["generated"][k].cpu().numpy() for k in ("path", "durations", "score", "status")}, want)
        tgt = out["target"]["durations"].cpu().numpy()
        assert tgt.sum(axis=1).tolist() == [23, 15, 9]
        groups = out["groups"].cpu().numpy()
        for name, g in (("bytes", None), ("chars", groups)):
            want_c, want_s = R.counts_batch(want["durations"], tgt, nb["input_lengths"], g)
            ok = want["status"] == R.OK
            assert np.array_equal(out[name]["counts"].cpu().numpy()[ok], want_c[ok])
            assert np.array_equal(out["status"].cpu().numpy() == R.OK, ok & (want_s == R.OK))
            assert np.array_equal(np.isnan(out[name]["rmse_ms"]), ~(ok & (want_s == R.OK)))
        got[align] = (out["generated"]["durations"].cpu().numpy(), _host(out["generated"]["layer"]), _host(out["generated"]["head"]))
    assert np.array_equal(got["reference"][0], got["hip"][0])              # the selected map is the map the per-layer list selects
    assert np.array_equal(got["reference"][1], got["hip"][1]) and np.array_equal(got["reference"][2], got["hip"][2])


def _host(v):
    return v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def test_command_line_extracts_teacher_durations(tiny, tmp_path, capsys):
    from b2s_hip import durations
    from utils.checkpoint import save_model
    from utils.text import text_to_byte_sequence
    m, _, hp = tiny
    rng = np.random.default_rng(9)
    names, texts, frames = ["spkA_0001", "spkB_0002", "spkA_0003"], ["hello wor", "grüße", "模型"], [23, 15, 9]
    data, model_dir = tmp_path / "data", tmp_path / "model"
    data.mkdir()
    model_dir.mkdir()
    with zipfile.ZipFile(data / "mels.zip", "w") as z:
        for n, t in zip(names, frames):
            with z.open(n + ".npy", "w") as f:
                np.save(f, np.clip(rng.standard_normal((t, hp.num_mels)), -4, 4).astype(np.float32))
    lines = ["%s.npy|%d|%s|%s\n" % (n, t, text, lang) for n, t, text, lang in zip(names, frames, texts, ["en-us", "de-de", "en-us"])]
    lines.append("spkA_0004.npy|12|listed without a mel|en-us\n")
    (data / "metadata.eval.txt").write_text("".join(lines), encoding="utf-8")
    (data / "lang_id.json").write_text(json.dumps({"en-us": 0, "de-de": 1}))
    (data / "spk_id.json").write_text(json.dumps({"spkA": 0, "spkB": 1}))
    ckpt = save_model(str(model_dir), m, step=5)
    for units in ("bytes", "chars"):
        out = tmp_path / units
        assert durations.main([ckpt, "--data-dir", str(data), "--out", str(out), "--batch", "2", "--units", units]) == 0
        printed = json.loads(capsys.readouterr().out)
        assert printed["utterances"] == 3 and printed["written"] == 3 and printed["units"] == units
        recs = [json.loads(line) for line in open(out / "durations.jsonl", encoding="utf-8")]
        assert [r["name"] for r in recs] == names
        for r, n, text, t in zip(recs, names, texts, frames):
            d = np.load(out / (n + ".npy"))
            n_bytes = len(text_to_byte_sequence(text))
            want_units = n_bytes if units == "bytes" else len(text) + 2
            assert d.dtype == np.int32 and d.shape == (want_units,) and int(d.sum()) == t and d.min() >= 1
            assert r["status"] == "OK" and r["frames"] == t and r["units"] == want_units
            assert 0 <= r["layer"] < 2 and 0 <= r["head"] < 2 and 0.0 < r["mono_focus"] <= r["focus"] + 1e-12
        assert not (out / "spkA_0004.npy").exists()
    by_byte = [np.load(tmp_path / "bytes" / (n + ".npy")) for n in names]
    by_char = [np.load(tmp_path / "chars" / (n + ".npy")) for n in names]
    for b, c, text in zip(by_byte, by_char, texts):
        g = R.code_point_groups(text_to_byte_sequence(text), len(b))
        assert c.tolist() == np.bincount(g, weights=b).astype(np.int64).tolist()
