"""CPU-only tests of the prosody targets' host side: the C ABI of libb2s_pros.so (declared, exported, bound, kept apart from the other
libraries; every host-side refusal without a GPU), the command line's usage errors, and the NumPy restatement (tests/pros_ref.py)
on properties known in closed form: the search against brute force over all state sequences, a planted track that frame-local YIN
loses and the search keeps, the contour and the unit sums."""
import ctypes as C
import itertools
import os
import re
import struct

import numpy as np
import pytest

import f0_ref
import pros_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = ["b2s_pros_energy", "b2s_pros_last_error", "b2s_pros_track", "b2s_pros_units", "b2s_pros_version", "b2s_pros_ws_bytes"]


# --------------------------------------------------------------------------------------------------------------------- the C ABI

def dynamic_symbols(path):
    """Names of the defined symbols in the .dynsym of a 64-bit little-endian ELF file."""
    data = open(path, "rb").read()
    assert data[:6] == b"\x7fELF\x02\x01"
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    names = []
    for _, sh_type, _, _, offset, size, link, _, _, entsize in sections:
        if sh_type != 11:                                                  # SHT_DYNSYM
            continue
        str_off = sections[link][4]
        for at in range(offset, offset + size, entsize):
            st_name, _, _, st_shndx = struct.unpack_from("<IBBH", data, at)
            if st_shndx != 0:
                names.append(data[str_off + st_name:data.index(b"\0", str_off + st_name)].decode())
    return names


def test_header_exports_and_prototypes_are_the_same_six_names():
    from b2s_hip import prosody
    l = prosody.load()
    header = open(os.path.join(ROOT, "include", "b2s_pros.h")).read()
    declared = sorted(set(re.findall(r"\b(b2s_pros_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert declared == prosody.EXPORTS == sorted(prosody._PROTOS) == ENTRY_POINTS
    assert sorted(n for n in dynamic_symbols(prosody.LIB_PATH) if n.startswith("b2s_")) == ENTRY_POINTS      # exactly these
    for name in ENTRY_POINTS:
        assert hasattr(l, name)
    assert l.b2s_pros_version() >= 100
    assert (prosody.OK, prosody.EMPTY, prosody.FAILED, prosody.SHORT, prosody.NOVOICE) == (0, 1, 2, 3, 4)
    assert (R.OK, R.EMPTY, R.FAILED, R.SHORT, R.NOVOICE) == (0, 1, 2, 3, 4)
    assert prosody.STATUS_NAMES == ("OK", "EMPTY", "FAILED", "SHORT", "NOVOICE")
    for name, value in (("OK", 0), ("EMPTY", 1), ("FAILED", 2), ("SHORT", 3), ("NOVOICE", 4), ("MAX_WIN", 2048), ("MAX_LAGS", 512),
                        ("MAX_W", 64), ("MAX_S", 1024)):
        assert re.search(r"#define B2S_PROS_%s %d\b" % (name, value), header)
    assert (prosody.MAX_WIN, prosody.MAX_LAGS, prosody.MAX_W, prosody.MAX_S) == (2048, 512, 64, 1024)


def test_the_binding_follows_the_shared_loader():
    """What test_cbind_host.py asks of the sibling bindings, asked of this one."""
    from b2s_hip import B2SError, cbind, durations, f0, lib, mcd, metrics, prosody, vocoder
    assert prosody.B2SError is cbind.B2SError is B2SError
    assert prosody.LIB_PATH == prosody._LIB.path and prosody.LIB_PATH.endswith("few-shot-transformer-tts_amd/libb2s_pros.so")
    assert prosody.EXPORTS == prosody._LIB.exports == sorted(prosody._PROTOS) and prosody._LIB.protos is prosody._PROTOS
    assert prosody.load() is prosody.load()                                # cached
    assert prosody.check(0) is None
    assert (prosody.OK, prosody.EMPTY, prosody.FAILED) == (cbind.OK, cbind.EMPTY, cbind.FAILED)
    for mod in (lib, vocoder, metrics, mcd, f0, durations):                # the other libraries do not grow
        assert not [n for n in mod.EXPORTS if n.startswith("b2s_pros")]
    protos = dict(prosody._PROTOS, b2s_pros_no_such_entry=(C.c_int, []))
    with pytest.raises(AttributeError, match="b2s_pros_no_such_entry"):
        cbind.Library("libb2s_pros.so", protos, "b2s_pros_last_error").load()
    # an error slot of its own: a refusal here does not show up in, or overwrite, the duration library's
    assert durations.load().b2s_dur_ws_bytes(2, 0, 10) == 0
    assert prosody.load().b2s_pros_ws_bytes(10, 0, 5) == 0
    with pytest.raises(B2SError, match=r"^tau_min must be >= 1 \(got 0\)$"):
        prosody.check(1)
    with pytest.raises(B2SError, match=r"^S must be in 1..1024 \(got 0\)$"):
        durations.check(1)
    with pytest.raises(B2SError, match=r"tau_min must be >= 1 \(got 0\)"):
        prosody.workspace(0, "cpu")                                        # 0 bytes is the library's refusal
    import torch
    ws = prosody.workspace(prosody.load().b2s_pros_ws_bytes(100, 32, 266), "cpu")
    assert ws.dtype == torch.uint8 and ws.numel() == 100 * 256 + 512


def test_readme_carries_the_entry_point_count():
    assert "`libb2s_pros.so`, %d entry points" % len(ENTRY_POINTS) in open(os.path.join(ROOT, "README.md")).read()


def test_importing_the_module_leaves_the_hyperparameters_alone():
    import hyperparams
    before = dict(hyperparams.DEFAULTS)
    from b2s_hip import prosody  # noqa: F401
    assert hyperparams.DEFAULTS == before
    assert not [k for k in hyperparams.DEFAULTS if k.startswith("pros") or k.startswith("pitch")]


def test_host_side_refusals_come_back_as_messages_without_a_gpu():
    from b2s_hip import prosody
    l = prosody.load()

    def err():
        return l.b2s_pros_last_error().decode()
    d = C.c_void_p(16)                   # never dereferenced: every call below fails its checks before a launch

    assert l.b2s_pros_ws_bytes(64000, 32, 266) == 64000 * 256 + 256256     # 235 lags: rows of 256 bytes; 64001 int32 rounded to 256
    assert l.b2s_pros_ws_bytes(0, 2, 9) == 256 and l.b2s_pros_ws_bytes(1, 2, 65) == 256 + 256
    assert l.b2s_pros_ws_bytes(3, 2, 66) == 3 * 128 + 128 + 256            # 65 lags: two waves
    assert l.b2s_pros_ws_bytes(-1, 2, 9) == 0 and "total_frames must be >= 0 (got -1)" in err()
    assert l.b2s_pros_ws_bytes(5, 0, 9) == 0 and "tau_min must be >= 1 (got 0)" in err()
    assert l.b2s_pros_ws_bytes(5, 9, 8) == 0 and "tau_max must be >= tau_min (got 8 and 9)" in err()
    assert l.b2s_pros_ws_bytes(5, 1, 513) == 0 and "at most 512 lags" in err()
    assert l.b2s_pros_ws_bytes(5, 1, 512) > 0

    eg = dict(pcm=d, lens=d, off=d, total=10, B=2, Lmax=1000, win=800, hop=200, energy=d, status=d)

    def energy(**over):
        v = dict(eg, **over)
        return l.b2s_pros_energy(v["pcm"], v["lens"], v["off"], v["total"], v["B"], v["Lmax"], v["win"], v["hop"], v["energy"],
                                 v["status"], None)
    for bad in (0, -1):
        assert energy(B=bad) != 0 and "B must be > 0 (got %d)" % bad in err()
    assert energy(B=65536) != 0 and "split the batch" in err()
    assert energy(Lmax=-1) != 0 and "Lmax must be >= 0 (got -1)" in err()
    assert energy(total=-1) != 0 and "total_frames must be >= 0 (got -1)" in err()
    for bad in (0, 2049):
        assert energy(win=bad) != 0 and "win must be in 1..2048 (got %d)" % bad in err()
    assert energy(hop=0) != 0 and "hop must be >= 1 (got 0)" in err()
    for name in ("lens", "off", "status"):
        assert energy(**{name: None}) != 0 and "lengths, frame_offsets or status is NULL" in err()
    for name in ("pcm", "energy"):
        assert energy(**{name: None}) != 0 and "pcm or energy is NULL" in err()

    need = l.b2s_pros_ws_bytes(10, 32, 266)
    tg = dict(cmnd=d, energy=d, floor=0, off=d, total=10, B=2, K=267, tau_min=32, tau_max=266, sr=16000.0, u=0.3, v=0.1, lam=0.02,
              mu=0.0005, W=8, tau=d, f0=d, score=d, status=d, ws=d, nbytes=need)

    def track(**over):
        v = dict(tg, **over)
        return l.b2s_pros_track(v["cmnd"], v["energy"], v["floor"], v["off"], v["total"], v["B"], v["K"], v["tau_min"], v["tau_max"],
                                v["sr"], v["u"], v["v"], v["lam"], v["mu"], v["W"], v["tau"], v["f0"], v["score"], v["status"],
                                v["ws"], v["nbytes"], None)
    for bad in (0, -3):
        assert track(B=bad) != 0 and "B must be > 0 (got %d)" % bad in err()
    assert track(total=-1) != 0 and "total_frames must be >= 0" in err()
    assert track(tau_min=0) != 0 and "tau_min must be >= 1 (got 0)" in err()
    assert track(tau_max=31) != 0 and "tau_max must be >= tau_min" in err()
    for bad in (266, 10):
        assert track(K=bad) != 0 and "K must be > tau_max (got %d and 266)" % bad in err()
    for bad in (-1, 65):
        assert track(W=bad) != 0 and "W must be in 0..64 (got %d)" % bad in err()
    for name in ("sr", "u", "v", "lam", "mu"):
        for bad in (float("nan"), float("inf")):
            assert track(**{name: bad}) != 0 and "must be finite" in err()
    for name in ("off", "score", "status"):
        assert track(**{name: None}) != 0 and "frame_offsets, score or status is NULL" in err()
    for name in ("cmnd", "energy", "tau", "f0"):
        assert track(**{name: None}) != 0 and "cmnd, energy, tau or f0 is NULL" in err()
    assert track(nbytes=need - 1) != 0 and "workspace of %d bytes, %d needed" % (need - 1, need) in err()
    assert track(ws=None) != 0 and "workspace of 0 bytes, %d needed" % need in err()
    assert track(ws=C.c_void_p(18)) != 0 and "4-byte aligned" in err()

    ug = dict(f0=d, tau=d, energy=d, off=d, total=10, dur=d, n_in=d, groups=None, B=2, S=64, cont=d, frames=d, voiced=d, vsum=d,
              csum=d, esum=d, units=d, status=d, ws=d, nbytes=40)

    def units(**over):
        v = dict(ug, **over)
        return l.b2s_pros_units(v["f0"], v["tau"], v["energy"], v["off"], v["total"], v["dur"], v["n_in"], v["groups"], v["B"], v["S"],
                                v["cont"], v["frames"], v["voiced"], v["vsum"], v["csum"], v["esum"], v["units"], v["status"], v["ws"],
                                v["nbytes"], None)
    for bad in (0, -7):
        assert units(B=bad) != 0 and "B must be > 0 (got %d)" % bad in err()
    for bad in (0, 1025):
        assert units(S=bad) != 0 and "S must be in 1..1024 (got %d)" % bad in err()
    assert units(total=-2) != 0 and "total_frames must be >= 0 (got -2)" in err()
    for name in ("off", "dur", "n_in"):
        assert units(**{name: None}) != 0 and "frame_offsets, durations or input_lengths is NULL" in err()
    for name in ("f0", "tau", "energy", "cont"):
        assert units(**{name: None}) != 0 and "f0, tau, energy or cont is NULL" in err()
    for name in ("frames", "voiced", "vsum", "csum", "esum", "units", "status"):
        assert units(**{name: None}) != 0 and "an output is NULL" in err()
    assert units(nbytes=39) != 0 and "workspace of 39 bytes, 40 needed" in err()
    assert units(ws=None) != 0 and "workspace of 0 bytes, 40 needed" in err()
    assert units(ws=C.c_void_p(18)) != 0 and "4-byte aligned" in err()


def test_there_is_no_cpu_fallback(monkeypatch):
    import torch
    from b2s_hip import prosody
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(prosody.B2SError, match="runs on the GPU only"):
        prosody.energy_batch(np.zeros((1, 400), np.int16), [400], win=800, hop=200)
    with pytest.raises(prosody.B2SError, match="runs on the GPU only"):
        prosody.prosody_targets(np.zeros((1, 3, 80), np.float32), [3], np.ones((1, 2), np.int32), [2])


def test_track_params_defaults_and_refusals():
    import hyperparams
    from b2s_hip import f0, prosody
    hyperparams.hparams.override_from_dict(hyperparams.DEFAULTS)
    prm = prosody.track_params()
    assert {k: prm[k] for k in R.DEFAULTS} == R.DEFAULTS
    assert prm["floor"] == f0.yin_params()["min_energy"] == f0_ref.min_energy(hyperparams.hparams.win_length, -40.0)
    assert prosody.track_params(u=1, W=3, floor=7) == {"u": 1.0, "v": 0.1, "lam": 0.02, "mu": 0.0005, "W": 3, "floor": 7}
    for bad, text in ((dict(W=65), "W must be in 0..64"), (dict(W=-1), "W must be in 0..64"), (dict(lam=float("nan")), "lam must be finite"),
                      (dict(v=float("inf")), "v must be finite"), (dict(threshold=0.1), "unknown track parameter")):
        with pytest.raises(prosody.B2SError, match=text):
            prosody.track_params(**bad)


def test_command_line_usage_errors_are_nonzero(tmp_path, capsys):
    import hyperparams
    from b2s_hip import prosody
    hyperparams.hparams.override_from_dict(hyperparams.DEFAULTS)
    ckpt = tmp_path / "model.ckpt-1"
    ckpt.write_bytes(b"not read before the usage checks")
    out = str(tmp_path / "out")
    assert prosody.main([str(tmp_path / "nowhere"), "--data-dir", str(tmp_path), "--out", out]) == 2       # no checkpoint
    assert "checkpoint not found" in capsys.readouterr().err
    assert prosody.main([str(ckpt), "--data-dir", str(tmp_path), "--out", out]) == 2                       # no mels.zip there
    assert "mels.zip not found" in capsys.readouterr().err
    assert prosody.main([str(ckpt), "--data-dir", str(tmp_path), "--out", out, "--batch", "0"]) == 2
    assert "--batch must be >= 1" in capsys.readouterr().err
    assert prosody.main([str(ckpt), "--data-dir", str(tmp_path), "--out", out, "--units", "words"]) == 2
    assert "--units must be" in capsys.readouterr().err
    assert prosody.main([str(ckpt), "--data-dir", str(tmp_path), "--out", out, "--n-iter", "-1"]) == 2
    assert "--n-iter must be >= 0" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        prosody.main([])
    assert e.value.code == 2
    capsys.readouterr()
    assert not os.path.exists(out)


def test_unit_stats_over_the_units_with_frames():
    from b2s_hip import prosody
    rows = [("en", [2, 0, 3], [100.0, 0.0, 200.0], [4.0, 0.0, 16.0]), ("de", [1, 1], [0.0, 50.0], [0.0, 8.0])]
    s = prosody.unit_stats(rows, win=800)
    o = s["overall"]
    assert o["pitch"]["count"] == 4 and o["pitch"]["mean"] == 87.5 and o["pitch"]["min"] == 0.0 and o["pitch"]["max"] == 200.0
    assert o["log_pitch"]["count"] == 3 and o["log_pitch"]["max"] == float(np.log(200.0))
    assert o["energy"]["count"] == 4 and o["energy"]["mean"] == 7.0
    assert o["energy_db"]["count"] == 3 and o["energy_db"]["min"] == float(10.0 * np.log10(4.0 / (800.0 * 32767.0 ** 2)))
    assert sorted(s["languages"]) == ["de", "en"] and s["languages"]["en"]["pitch"]["count"] == 2
    assert s["languages"]["de"]["log_pitch"] == {"count": 1, "mean": float(np.log(50.0)), "std": 0.0, "min": float(np.log(50.0)),
                                                 "max": float(np.log(50.0))}
    assert prosody.unit_stats([], 800)["overall"]["pitch"] == {"count": 0, "mean": None, "std": None, "min": None, "max": None}


# ------------------------------------------------------------------------------------------------------------------- the search

def brute_force(cmnd, gated, tau_min, tau_max, prm):
    """(cost, states) of the first minimal sequence: the sequences are visited so that the one whose last state comes first in the
    order 0, tau_min, .., tau_max, then whose state before that does, ... is met first, and only a strictly smaller cost replaces."""
    states = [0] + list(range(tau_min, tau_max + 1))
    best, best_seq = None, None
    for rev in itertools.product(states, repeat=len(cmnd)):                # rev[0] is the last frame's state
        seq = rev[::-1]
        W = prm["W"]
        if any(a and b and abs(a - b) > W for a, b in zip(seq, seq[1:])):
            continue
        cost = R.path_cost(cmnd, gated, seq, tau_min, prm["u"], prm["v"], prm["lam"], prm["mu"])
        if best is None or cost < best:
            best, best_seq = cost, seq
    return best, list(best_seq)


def test_the_search_equals_brute_force_over_all_state_sequences():
    """T = 4 with the states {0, 2, 3, 4}: 256 sequences.  Half of the 50 tables hold multiples of 1/4 with power-of-two parameters,
    so that many sequences cost exactly the same and the tie rule picks the path; the others are uniform random."""
    rng = np.random.default_rng(50)
    ties = 0
    for case in range(50):
        T, tau_min, tau_max = 4, 2, 4
        if case % 2:
            cm = rng.integers(0, 3, size=(T, tau_max + 1)).astype(np.float64) / 4
            prm = {"u": 0.5, "v": 0.25, "lam": 0.25, "mu": 0.125, "W": 1 + case % 3}
        else:
            cm = rng.random((T, tau_max + 1)) * 2
            prm = dict(R.DEFAULTS, W=1 + case % 2)
        energy = [0 if (case % 5 == 0 and t == case % 4) else 10 for t in range(T)]
        got = R.track(cm, energy, 5, tau_min, tau_max, **prm)
        cost, seq = brute_force(cm, [e < 5 for e in energy], tau_min, tau_max, prm)
        assert got["status"] == R.OK
        assert np.float64(got["score"]).view(np.int64) == np.float64(cost).view(np.int64), case
        assert got["tau"].tolist() == seq, case
        if case % 2:
            costs = [R.path_cost(cm, [e < 5 for e in energy], s[::-1], tau_min, prm["u"], prm["v"], prm["lam"], prm["mu"])
                     for s in itertools.product([0, 2, 3, 4], repeat=T)
                     if not any(a and b and abs(a - b) > prm["W"] for a, b in zip(s, s[1:]))]
            ties += sum(c == cost for c in costs) > 1
    assert ties >= 10                                                      # the tie rule was at work


def test_the_oracle_statuses_and_gates():
    cm = np.full((3, 6), 0.05)
    r = R.track(cm[:0], [], 0, 2, 5)
    assert r["status"] == R.EMPTY and r["score"] == 0.0 and len(r["tau"]) == 0
    bad = cm.copy()
    bad[1, 3] = np.nan
    r = R.track(bad, [9, 9, 9], 0, 2, 5)
    assert r["status"] == R.FAILED and not r["tau"].any() and not r["f0"].any() and np.isnan(r["score"])
    bad[1, 3], bad[1, 0] = 0.05, np.inf                                    # below tau_min: not looked at
    assert R.track(bad, [9, 9, 9], 0, 2, 5)["status"] == R.OK
    r = R.track(cm, [0, 0, 0], 1, 2, 5)                                    # every frame gated: all unvoiced
    assert r["status"] == R.OK and not r["tau"].any() and r["score"] == float(np.float64(0.3) + 0.3 + 0.3)
    r = R.track(cm, [9, 0, 9], 1, 2, 5)
    assert r["tau"][1] == 0 and r["tau"][0] > 0 and r["tau"][2] > 0       # 0.05 + bias is cheaper than u = 0.3 even after 2 v


def test_a_planted_track_is_kept_where_frame_local_yin_loses_it():
    wav, f = R.planted_signal()
    pcm, _, st = f0_ref.quantize(wav)
    assert st == f0_ref.OK
    floor = f0_ref.min_energy(800, -40)
    y = f0_ref.yin(pcm, floor=floor)
    tr = R.track(y["cmnd"], y["energy"], floor, 32, 266, **R.DEFAULTS)
    assert tr["status"] == R.OK and len(tr["tau"]) == 61
    noisy = np.arange(36, 60)
    assert not y["tau"][noisy].any()                                       # raw YIN voices none of them
    want = np.round(16000.0 / f[np.minimum(noisy * 200, len(f) - 1)]).astype(int)
    assert np.all(tr["tau"][noisy] > 0) and np.all(np.abs(tr["tau"][noisy] - want) <= 2)
    pause = np.arange(22, 28)
    assert not y["tau"][pause].any() and not tr["tau"][pause].any()
    for t in np.nonzero(tr["tau"] > 0)[0]:                                 # no frame sits at a doubled lag
        ideal = 16000.0 / f[min(t * 200, len(f) - 1)]
        assert abs(tr["tau"][t] - 2 * ideal) > 4
    voiced = tr["tau"] > 0
    lag = tr["tau"][voiced].astype(np.float64)                             # the refinement moves a lag by at most one
    assert np.all(tr["f0"][voiced] >= 16000.0 / (lag + 1)) and np.all(tr["f0"][voiced] <= 16000.0 / (lag - 1))


# ----------------------------------------------------------------------------------------------------- energy, contour and units

def test_energy_in_closed_form():
    pcm = np.full(1000, 3, np.int16)
    e = R.energy(pcm, 800, 200)
    assert e.tolist() == [9 * 400, 9 * 600, 9 * 800, 9 * 800, 9 * 600, 9 * 400]
    assert R.energy(np.zeros(0, np.int16), 800, 200).tolist() == [0]
    assert R.energy(np.full(5, -32768, np.int16), 16, 4).tolist() == [5 * 2 ** 30, 5 * 2 ** 30]
    y = f0_ref.yin(np.arange(-300, 300).astype(np.int16), win=16, hop=4, tau_min=2, tau_max=9)
    assert len(R.energy(np.arange(600), 16, 4)) == len(y["tau"])          # YIN's frame count


def test_contour_interpolates_and_holds_the_ends():
    f0 = np.array([0, 0, 100.0, 0, 0, 0, 140.0, 150.0, 0, 0])
    tau = (f0 > 0).astype(np.int32) * 50
    c = R.contour(f0, tau, 10)
    assert c.tolist() == [100.0, 100.0, 100.0, 110.0, 120.0, 130.0, 140.0, 150.0, 150.0, 150.0]
    assert np.all(np.diff(c[2:7]) > 0)                                     # a gap is monotonic between its ends
    assert R.contour(f0, tau, 5).tolist() == [100.0] * 5 + [0.0] * 5       # frames from n on are not looked at
    assert R.contour(f0, tau, 2) is None and R.contour(f0, np.zeros(10, np.int32), 10) is None
    rng = np.random.default_rng(2)
    for _ in range(20):
        f = rng.random(40) * 200 + 60
        v = rng.random(40) < 0.3
        v[rng.integers(0, 40)] = True
        c = R.contour(np.where(v, f, 0.0), v.astype(np.int32), 40)
        idx = np.nonzero(v)[0]
        for a, b in zip(idx, idx[1:]):
            seg = c[a:b + 1]
            assert np.all(np.diff(seg) >= 0) or np.all(np.diff(seg) <= 0)
            assert min(f[a], f[b]) <= seg.min() and seg.max() <= max(f[a], f[b])


def test_unit_sums_properties_and_statuses():
    rng = np.random.default_rng(3)
    F, S = 50, 9
    f0 = np.full(F, 123.25)
    tau = np.full(F, 130, np.int32)
    en = rng.integers(0, 2 ** 40, size=F)
    d = np.array([5, 0, 7, 1, 9, 3, 0, 0, 99], np.int32)
    r = R.units(f0, tau, en, d, 8)
    assert r["status"] == R.OK and r["units"] == 8 and r["frames"].sum() == d[:8].sum() == 25
    m = R.means(r)
    assert np.all(m["pitch"][r["frames"] > 0] == 123.25) and np.all(m["pitch_voiced"][r["frames"] > 0] == 123.25)   # a constant track
    assert np.all(m["pitch"][r["frames"] == 0] == 0) and r["energy_sum"][:8].sum() == en[:25].sum() and r["frames"][8] == 0
    assert r["f0_cont_sum"][1] == 0 and r["voiced"][1] == 0 and np.all(r["cont"][25:] == 0)
    g = np.array([0, 0, 1, 2, 2, 2, 3, 3, -1], np.int32)
    rg = R.units(f0, tau, en, d, 8, g)
    assert rg["units"] == 4 and rg["frames"][:4].tolist() == [5, 7, 13, 0] and rg["frames"].sum() == 25
    assert rg["energy_sum"][2] == en[12:25].sum()
    tau2 = tau.copy()
    tau2[3:20] = 0                                                         # a gap over several units
    r2 = R.units(np.where(tau2 > 0, f0, 0.0), tau2, en, d, 8)
    assert r2["voiced"][:4].tolist() == [3, 0, 0, 0] and R.means(r2)["pitch"][2] == 123.25 and R.means(r2)["pitch_voiced"][2] == 0
    assert R.units(f0, tau, en, d, 9)["status"] == R.SHORT                 # 124 frames asked of 50
    assert R.units(f0, tau, en, d, 0)["status"] == R.EMPTY and R.units(f0, tau, en, d, 10)["status"] == R.FAILED
    neg = d.copy()
    neg[2] = -1
    assert R.units(f0, tau, en, neg, 8)["status"] == R.FAILED
    for bad in ([1, 1, 2, 3, 4, 5, 6, 7, 8], [0, 2, 2, 3, 4, 5, 6, 7, 8], [0, 1, 0, 1, 2, 3, 4, 5, 6]):
        assert R.units(f0, tau, en, d, 8, np.array(bad))["status"] == R.FAILED
    nv = R.units(f0, np.zeros(F, np.int32), en, d, 8)
    assert nv["status"] == R.NOVOICE and not nv["cont"].any() and nv["energy_sum"][:8].sum() == en[:25].sum() and nv["units"] == 8
    exact = R.units(f0, tau, en, np.array([20, 30], np.int32), 2)          # n == F
    assert exact["status"] == R.OK and exact["frames"].tolist() == [20, 30]
