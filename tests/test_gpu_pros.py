"""GPU tests of the prosody targets (b2s_hip.prosody, libb2s_pros.so) against the NumPy restatement tests/pros_ref.py.

The gate is equality throughout: integers EQUAL, fp64 compared as int64 bit patterns.  Every operation of the three calls is
specified (include/b2s_pros.h), so there is no tolerance to derive: anything but equality is a defect.  Every output is pre-filled
with a sentinel and has guard rows behind it, and so has the workspace; those must stay untouched."""
import json
import zipfile

import numpy as np
import pytest
import torch

import dur_ref
import f0_ref
import pros_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
TIE = {"u": 0.5, "v": 0.25, "lam": 2.0 ** -10, "mu": 2.0 ** -10}   # powers of two: on a table of quarters every sum is exact


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def offsets(counts):
    return np.concatenate(([0], np.cumsum(counts))).astype(np.int32)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(DEV)


# ------------------------------------------------------------------------------------------------------------------------ energy

def run_energy(rows, win, hop, guard=3):
    """b2s_pros_energy through the C ABI on a list of int16 arrays -> (energy per row, status)."""
    from b2s_hip import prosody
    l = prosody.load()
    n = [len(r) for r in rows]
    B, Lmax = len(rows), max(n + [1])
    pcm = np.full((B, Lmax), 12345, np.int16)                              # past a length: never read
    for i, r in enumerate(rows):
        pcm[i, :n[i]] = r
    frames = [1 + v // hop for v in n]
    off = offsets(frames)
    total = int(off[-1])
    e = torch.full((total + guard,), -7, dtype=torch.int64, device=DEV)
    st = torch.full((B + guard,), -7, dtype=torch.int32, device=DEV)
    p, ln, o = dev(pcm, np.int16), dev(n, np.int32), dev(off, np.int32)
    prosody.check(l.b2s_pros_energy(p.data_ptr(), ln.data_ptr(), o.data_ptr(), total, B, Lmax, win, hop, e.data_ptr(), st.data_ptr(),
                                    None))
    torch.cuda.synchronize()
    e, st = e.cpu().numpy(), st.cpu().numpy()
    assert np.all(e[total:] == -7) and np.all(st[B:] == -7)
    return [e[off[i]:off[i + 1]] for i in range(B)], st[:B]


@pytest.mark.parametrize("win,hop,lengths", [(800, 200, [0, 1, 199, 200, 201, 399, 1000, 4007]), (16, 4, [0, 3, 4, 5, 64, 65, 257])])
def test_energy_equals_the_oracle(win, hop, lengths):
    rng = np.random.default_rng(win)
    rows = [rng.integers(-32768, 32768, size=n).astype(np.int16) for n in lengths]
    rows.append(np.full(lengths[-1], -32768, np.int16))                    # 2^30 per sample: a 32-bit partial sum would overflow
    got, st = run_energy(rows, win, hop)
    assert np.all(st == R.OK)
    for r, g in zip(rows, got):
        assert np.array_equal(g, R.energy(r, win, hop))
    assert got[-1].max() == min(win, lengths[-1]) * 2 ** 30
    alone, _ = run_energy(rows[-2:-1], win, hop)                           # alone or in the batch
    assert np.array_equal(alone[0], got[-2])


def test_energy_python_surface_and_bad_offsets():
    from b2s_hip import prosody
    rng = np.random.default_rng(6)
    rows = [rng.integers(-3000, 3000, size=n).astype(np.int16) for n in (1000, 0, 437)]
    out = prosody.energy_batch(rows, win=800, hop=200)
    assert out["energy"].is_cuda and out["energy"].dtype == torch.int64 and out["frames"] == [6, 1, 3]
    assert out["frame_offsets"].tolist() == [0, 6, 7, 10] and out["status"].cpu().tolist() == [0, 0, 0]
    e = out["energy"].cpu().numpy()
    for i, r in enumerate(rows):
        assert np.array_equal(e[out["frame_offsets"][i]:out["frame_offsets"][i + 1]], R.energy(r, 800, 200))
    wav = (rows[0].astype(np.float32) / 3000.0)[None]                      # not int16: quantised first
    q = prosody.energy_batch(wav, [1000], win=800, hop=200)
    assert np.array_equal(q["energy"].cpu().numpy(), R.energy(f0_ref.quantize(wav[0])[0], 800, 200))
    # offsets that do not fit the lengths: FAILED, and nothing of that row is written
    l = prosody.load()
    pcm, ln = dev(np.zeros((2, 400), np.int16) + 5, np.int16), dev([400, 400], np.int32)
    off = dev([0, 3, 7], np.int32)                                         # 3 frames at hop 200 are right, 4 are not
    en = torch.full((9,), -7, dtype=torch.int64, device=DEV)
    st = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    prosody.check(l.b2s_pros_energy(pcm.data_ptr(), ln.data_ptr(), off.data_ptr(), 7, 2, 400, 800, 200, en.data_ptr(), st.data_ptr(), None))
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [R.OK, R.FAILED] and en.cpu().tolist()[3:] == [-7] * 6 and en.cpu().tolist()[:3] == [25 * 400] * 3


# ------------------------------------------------------------------------------------------------------------------------- track

FRAMES = [1, 2, 3, 17, 64, 65, 130]
RANGES = [(2, 9), (2, 63), (2, 64), (32, 266)]      # one wave partly filled, 62 and 63 lags (the 64 / 65 state edge), 235 lags
CONTENTS = ["yin", "uniform", "gated", "allgated"]
FLOOR = 1000


def yin_cmnd(T, tau_min, tau_max, seed):
    """CMND and energies of f0_ref.yin on a short harmonic signal with a pause: T frames."""
    win, hop = (16, 4) if tau_max < 16 else (64, 16)
    rng = np.random.default_rng(seed)
    n = hop * (T - 1) + 1
    period = rng.uniform(tau_min + 1, min(tau_max, 4 * win) - 1)
    x = 8000 * np.sin(2 * np.pi * np.arange(n) / period) + 3000 * np.sin(4 * np.pi * np.arange(n) / period + 1) + 300 * rng.standard_normal(n)
    x[n // 3:n // 3 + n // 5] = 0
    y = f0_ref.yin(np.rint(x).astype(np.int16), win=win, hop=hop, tau_min=tau_min, tau_max=tau_max, floor=FLOOR)
    assert len(y["tau"]) == T
    return y["cmnd"], np.array(y["energy"], np.int64)


def make_case(kind, T, tau_min, tau_max, seed):
    """(cmnd [T, tau_max + 1], energy [T]) of one utterance."""
    rng = np.random.default_rng(seed)
    K = tau_max + 1
    en = np.full(T, FLOOR + 5, np.int64)
    if kind == "yin":
        return yin_cmnd(T, tau_min, tau_max, seed)
    if kind == "tie":
        cm = rng.integers(0, 3, size=(T, K)).astype(np.float64) / 4
        en[rng.random(T) < 0.2] = FLOOR - 1
        return cm, en
    cm = rng.random((T, K)) * 2
    if kind == "uniform":
        cm[:, rng.integers(tau_min, tau_max + 1)] *= 0.02                  # one cheap lag, so that there is something to follow
    if kind == "gated":                                                    # off at the start, the end and every third frame
        cm *= 0.05
        en[0] = en[T - 1] = FLOOR - 1
        en[::3] = FLOOR - 1
    if kind == "allgated":
        en[:] = 0
    return cm, en


_track_cache = {}


def track_batch_case(rng_key, tau_min, tau_max, W, tie):
    """Seven utterances (FRAMES) with rotated contents, and the oracle's results: computed once, left unchanged."""
    key = (rng_key, tau_min, tau_max, W, tie)
    if key not in _track_cache:
        prm = dict(R.DEFAULTS, W=W, **(TIE if tie else {}))
        cases = []
        for i, T in enumerate(FRAMES):
            kind = "tie" if tie else CONTENTS[(i + rng_key) % len(CONTENTS)]
            cases.append(make_case(kind, T, tau_min, tau_max, 1000 * tau_max + 10 * T + rng_key))
        want = [R.track(cm, en, FLOOR, tau_min, tau_max, **prm) for cm, en in cases]
        _track_cache[key] = (cases, prm, want)
    return _track_cache[key]


def run_track(cases, tau_min, tau_max, prm, floor=FLOOR, guard=3):
    """b2s_pros_track through the C ABI on a list of (cmnd, energy) -> per utterance dicts of host arrays."""
    from b2s_hip import prosody
    l = prosody.load()
    B, K = len(cases), tau_max + 1
    off = offsets([len(c[0]) for c in cases])
    total = int(off[-1])
    cm = dev(np.concatenate([c[0] for c in cases]).reshape(total, K), np.float64)
    en = dev(np.concatenate([c[1] for c in cases]), np.int64)
    tau = torch.full((total + guard,), -7, dtype=torch.int32, device=DEV)
    f0 = torch.full((total + guard,), -12345.0, dtype=torch.float64, device=DEV)
    score = torch.full((B + guard,), -12345.0, dtype=torch.float64, device=DEV)
    st = torch.full((B + guard,), -7, dtype=torch.int32, device=DEV)
    nbytes = l.b2s_pros_ws_bytes(total, tau_min, tau_max)
    ws = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    o = dev(off, np.int32)
    prosody.check(l.b2s_pros_track(cm.data_ptr(), en.data_ptr(), floor, o.data_ptr(), total, B, K, tau_min, tau_max, 16000.0, prm["u"],
                                   prm["v"], prm["lam"], prm["mu"], prm["W"], tau.data_ptr(), f0.data_ptr(), score.data_ptr(),
                                   st.data_ptr(), ws.data_ptr(), nbytes, None))
    torch.cuda.synchronize()
    tau, f0, score, st = tau.cpu().numpy(), f0.cpu().numpy(), score.cpu().numpy(), st.cpu().numpy()
    assert np.all(tau[total:] == -7) and np.all(f0[total:] == -12345.0) and np.all(score[B:] == -12345.0) and np.all(st[B:] == -7)
    assert np.all(ws[nbytes:].cpu().numpy() == 0xA5)
    return [{"tau": tau[off[i]:off[i + 1]], "f0": f0[off[i]:off[i + 1]], "score": float(score[i]), "status": int(st[i])} for i in range(B)]


def same_track(got, want):
    assert got["status"] == want["status"]
    assert np.array_equal(got["tau"], want["tau"])
    assert np.array_equal(bits(got["f0"]), bits(want["f0"]))
    if np.isnan(want["score"]):
        assert np.isnan(got["score"])
    else:
        assert bits(got["score"]) == bits(want["score"])


@pytest.mark.parametrize("tie", [False, True])
@pytest.mark.parametrize("W", [1, 8, 64])
@pytest.mark.parametrize("tau_min,tau_max", RANGES)
def test_track_equals_the_oracle(tau_min, tau_max, W, tie):
    cases, prm, want = track_batch_case(W, tau_min, tau_max, W, tie)
    got = run_track(cases, tau_min, tau_max, prm)
    voiced = 0
    for g, w_, (cm, en) in zip(got, want, cases):
        assert w_["status"] == R.OK
        same_track(g, w_)
        assert not g["tau"][en < FLOOR].any()                              # a gated frame is unvoiced
        voiced += int((g["tau"] > 0).sum())
    assert voiced > 0
    if tie:                                                                # many cells have equal candidates: the tie rule decides
        assert sum(w_["ties"] for w_ in want) >= 50
    if not tie:
        kinds = [CONTENTS[(i + W) % len(CONTENTS)] for i in range(len(FRAMES))]
        assert set(kinds) == set(CONTENTS)
        for g, kind in zip(got, kinds):
            if kind == "allgated":                                         # all unvoiced, and OK
                assert not g["tau"].any() and not g["f0"].any()


def test_track_failed_rows_leave_the_neighbours_alone():
    tau_min, tau_max, prm = 2, 64, dict(R.DEFAULTS)
    cases = [make_case("uniform", 17, tau_min, tau_max, s) for s in range(5)]
    cases.append((np.zeros((0, tau_max + 1)), np.zeros(0, np.int64)))      # no frame: EMPTY
    cases[1][0][5, 40] = np.nan                                            # inside the lag range
    cases[2][0][16, 64] = np.inf
    cases[3][0][3, 1] = np.nan                                             # below tau_min: never looked at by the search
    cases[4][0][0, 2] = -np.inf
    cases[4][1][0] = 0                                                     # in a gated frame: FAILED all the same
    want = [R.track(cm, en, FLOOR, tau_min, tau_max, **prm) for cm, en in cases]
    assert [w_["status"] for w_ in want] == [R.OK, R.FAILED, R.FAILED, R.OK, R.FAILED, R.EMPTY]
    got = run_track(cases, tau_min, tau_max, prm)
    for g, w_ in zip(got, want):
        same_track(g, w_)
    for i in (1, 2, 4):
        assert not got[i]["tau"].any() and not got[i]["f0"].any() and np.isnan(got[i]["score"])
    assert got[5]["score"] == 0.0
    for i in (0, 3):                                                       # bit-identical to their run alone
        alone = run_track(cases[i:i + 1], tau_min, tau_max, prm)[0]
        same_track(alone, got[i])
    # offsets that decrease: FAILED, nothing of the row is written
    from b2s_hip import prosody
    l = prosody.load()
    cm, en = dev(cases[0][0], np.float64), dev(cases[0][1], np.int64)
    off = dev([0, 17, 5], np.int32)
    tau = torch.full((17,), -7, dtype=torch.int32, device=DEV)
    f0 = torch.full((17,), -1.0, dtype=torch.float64, device=DEV)
    score = torch.full((2,), -1.0, dtype=torch.float64, device=DEV)
    st = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    nbytes = l.b2s_pros_ws_bytes(17, tau_min, tau_max)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    prosody.check(l.b2s_pros_track(cm.data_ptr(), en.data_ptr(), FLOOR, off.data_ptr(), 17, 2, tau_max + 1, tau_min, tau_max, 16000.0,
                                   0.3, 0.1, 0.02, 0.0005, 8, tau.data_ptr(), f0.data_ptr(), score.data_ptr(), st.data_ptr(),
                                   ws.data_ptr(), nbytes, None))
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [R.OK, R.FAILED] and np.array_equal(tau.cpu().numpy(), want[0]["tau"])


def test_track_alone_or_in_the_batch_and_from_run_to_run():
    tau_min, tau_max = 32, 266
    cases, prm, _ = track_batch_case(8, tau_min, tau_max, 8, False)
    a, b = run_track(cases, tau_min, tau_max, prm), run_track(cases, tau_min, tau_max, prm)
    for x, y in zip(a, b):
        same_track(x, y)
    for i in (3, 6):
        same_track(run_track(cases[i:i + 1], tau_min, tau_max, prm)[0], a[i])


# ------------------------------------------------------------------------------------------------------------------------- units

PATTERNS = ["all", "none", "first", "last", "alternate", "gaps"]


def voicing(kind, F, rng):
    v = np.zeros(F, bool)
    if kind == "all":
        v[:] = True
    elif kind == "first":
        v[0] = True
    elif kind == "last":
        v[F - 1] = True
    elif kind == "alternate":
        v[::2] = True
    elif kind == "gaps":                                                   # runs and gaps longer than most units
        t = 0
        while t < F:
            n = int(rng.integers(1, 12))
            v[t:t + n] = True
            t += n + int(rng.integers(3, 40))
    return v


def units_batch(S, seed):
    """Eight utterances at S positions: the six voicing patterns (n below F on even rows, n == F on odd ones), a SHORT row and a row
    with a negative duration; zero durations are planted from S = 2 on, and row 1 uses one position fewer than the batch holds."""
    rng = np.random.default_rng(seed)
    T = 3 * S + 5
    rows = []
    for i in range(8):
        kind = PATTERNS[i % len(PATTERNS)]
        n_in = max(1, S - 1) if i == 1 else S
        d = np.full(S, 77, np.int64)
        d[:n_in] = dur_ref.random_durations(rng, n_in, T)
        if n_in >= 2:                                                      # a position without a frame, its frames go to a neighbour
            z = int(rng.integers(0, n_in - 1))
            d[z + 1] += d[z]
            d[z] = 0
        F = T + (7 if i % 2 == 0 else 0)
        if i == 6:
            F = T - 1                                                      # SHORT
        if i == 7:
            d[n_in // 2] = -1
        v = voicing(kind, F, rng)
        if kind == "last":
            v[:] = False
            v[T - 1] = True                                                # the last frame the durations cover
        f0 = np.where(v, rng.uniform(60, 400, size=F), 0.0)
        tau = np.where(v, rng.integers(32, 267, size=F), 0).astype(np.int32)
        en = rng.integers(0, 2 ** 40, size=F).astype(np.int64)
        g = np.cumsum(rng.random(S) < 0.6).astype(np.int64)
        g -= g[0]
        g[n_in:] = -5
        rows.append({"f0": f0, "tau": tau, "energy": en, "dur": d.astype(np.int32), "n_in": n_in, "groups": g.astype(np.int32)})
    return rows


def run_units(rows, use_groups, guard=2):
    from b2s_hip import prosody
    l = prosody.load()
    B, S = len(rows), len(rows[0]["dur"])
    off = offsets([len(r["f0"]) for r in rows])
    total = int(off[-1])
    f0, tau = dev(np.concatenate([r["f0"] for r in rows]), np.float64), dev(np.concatenate([r["tau"] for r in rows]), np.int32)
    en = dev(np.concatenate([r["energy"] for r in rows]), np.int64)
    d, n_in = dev(np.stack([r["dur"] for r in rows]), np.int32), dev([r["n_in"] for r in rows], np.int32)
    g = dev(np.stack([r["groups"] for r in rows]), np.int32) if use_groups else None
    cont = torch.full((total + guard,), -12345.0, dtype=torch.float64, device=DEV)
    out = {"frames": torch.full((B + guard, S), -7, dtype=torch.int32, device=DEV),
           "voiced": torch.full((B + guard, S), -7, dtype=torch.int32, device=DEV),
           "f0_voiced_sum": torch.full((B + guard, S), -12345.0, dtype=torch.float64, device=DEV),
           "f0_cont_sum": torch.full((B + guard, S), -12345.0, dtype=torch.float64, device=DEV),
           "energy_sum": torch.full((B + guard, S), -7, dtype=torch.int64, device=DEV)}
    units = torch.full((B + guard,), -7, dtype=torch.int32, device=DEV)
    st = torch.full((B + guard,), -7, dtype=torch.int32, device=DEV)
    ws = torch.full((4 * total + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    o = dev(off, np.int32)
    prosody.check(l.b2s_pros_units(f0.data_ptr(), tau.data_ptr(), en.data_ptr(), o.data_ptr(), total, d.data_ptr(), n_in.data_ptr(),
                                   g.data_ptr() if use_groups else None, B, S, cont.data_ptr(), out["frames"].data_ptr(),
                                   out["voiced"].data_ptr(), out["f0_voiced_sum"].data_ptr(), out["f0_cont_sum"].data_ptr(),
                                   out["energy_sum"].data_ptr(), units.data_ptr(), st.data_ptr(), ws.data_ptr(), 4 * total, None))
    torch.cuda.synchronize()
    cont, units, st = cont.cpu().numpy(), units.cpu().numpy(), st.cpu().numpy()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    assert np.all(cont[total:] == -12345.0) and np.all(units[B:] == -7) and np.all(st[B:] == -7)
    assert np.all(ws[4 * total:].cpu().numpy() == 0xA5)
    for k, v in host.items():
        assert np.all(v[B:] == (-7 if v.dtype.kind == "i" else -12345.0)), k
    res = []
    for i in range(B):
        r = {k: v[i] for k, v in host.items()}
        r.update(cont=cont[off[i]:off[i + 1]], units=int(units[i]), status=int(st[i]))
        res.append(r)
    return res


def same_units(got, want):
    assert got["status"] == want["status"] and got["units"] == want["units"]
    for k in ("frames", "voiced", "energy_sum"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("cont", "f0_voiced_sum", "f0_cont_sum"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k


@pytest.mark.parametrize("use_groups", [False, True])
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 256])
def test_units_equal_the_oracle(S, use_groups):
    rows = units_batch(S, 40 + S)
    want = [R.units(r["f0"], r["tau"], r["energy"], r["dur"], r["n_in"], r["groups"] if use_groups else None) for r in rows]
    assert [w_["status"] for w_ in want] == [R.OK, R.NOVOICE, R.OK, R.OK, R.OK, R.OK, R.SHORT, R.FAILED]
    got = run_units(rows, use_groups)
    for g, w_, r in zip(got, want, rows):
        same_units(g, w_)
        if w_["status"] in (R.OK, R.NOVOICE):
            assert g["frames"].sum() == r["dur"][:r["n_in"]].sum() == 3 * S + 5
    assert not got[1]["cont"].any() and got[1]["energy_sum"].sum() == rows[1]["energy"][:3 * S + 5].sum()
    alone = run_units(rows[5:6], use_groups)[0]                            # alone or in the batch
    same_units(alone, got[5])


def test_units_statuses_of_lengths_and_groups():
    rows = units_batch(6, 1)[:6]
    rows[0]["n_in"] = 0                                                    # EMPTY
    rows[1]["n_in"] = 7                                                    # outside 0..S
    rows[2]["groups"] = np.array([1, 1, 2, 3, 4, 5], np.int32)             # starts above 0
    rows[3]["groups"] = np.array([0, 2, 2, 3, 4, 5], np.int32)             # skips a value
    rows[4]["groups"] = np.array([0, 1, 0, 1, 2, 3], np.int32)             # decreases
    want = [R.units(r["f0"], r["tau"], r["energy"], r["dur"], r["n_in"], r["groups"]) for r in rows]
    assert [w_["status"] for w_ in want] == [R.EMPTY, R.FAILED, R.FAILED, R.FAILED, R.FAILED, R.OK]
    for g, w_ in zip(run_units(rows, True), want):
        same_units(g, w_)


# -------------------------------------------------------------------------------------------------------------------- end to end

@pytest.fixture
def default_hp():
    import hyperparams
    from hyperparams import hparams as hp
    hp.override_from_dict(hyperparams.DEFAULTS)
    yield hp
    hp.override_from_dict(hyperparams.DEFAULTS)


def test_prosody_targets_with_waveforms_equal_the_restated_chain(default_hp):
    from b2s_hip import f0, prosody
    hp = default_hp
    win, hop = int(hp.win_length), int(hp.hop_length)
    rng = np.random.default_rng(12)
    wavs = []
    for n, hz in ((13 * hop, 140.0), (9 * hop + 57, 95.0), (5 * hop, 230.0)):
        t = np.arange(n) / float(hp.sr)
        x = 0.4 * np.sin(2 * np.pi * hz * t) + 0.2 * np.sin(4 * np.pi * hz * t + 0.5) + 0.01 * rng.standard_normal(n)
        x[n // 2:n // 2 + 2 * hop] *= 1e-4                                # a pause below the floor
        wavs.append(x.astype(np.float32))
    frames = [1 + len(w_) // hop for w_ in wavs]
    S = 5
    d = np.stack([dur_ref.random_durations(rng, S, f - (i == 1)) for i, f in enumerate(frames)]).astype(np.int32)   # row 1: n below F
    groups = np.array([[0, 0, 1, 2, 2]] * 3, np.int32)
    yp = f0.yin_params(hp)
    mels = np.zeros((3, max(frames), int(hp.num_mels)), np.float32)       # not looked at when the waveforms are given
    for g in (None, groups):
        out = prosody.prosody_targets(mels, frames, d, [S] * 3, groups=g, wavs=wavs, hp=hp)
        assert out["pitch"].is_cuda and out["status"].cpu().tolist() == [R.OK] * 3
        off = out["track"]["frame_offsets"]
        assert off.tolist() == offsets(frames).tolist()
        voiced_total = 0
        for i, w_ in enumerate(wavs):
            pcm = f0_ref.quantize(w_)[0]
            y = f0_ref.yin(pcm, win=win, hop=hop, tau_min=yp["tau_min"], tau_max=yp["tau_max"], floor=yp["min_energy"], sr=yp["sr"])
            en = R.energy(pcm, win, hop)
            tr = R.track(y["cmnd"], en, yp["min_energy"], yp["tau_min"], yp["tau_max"], sr=yp["sr"], **R.DEFAULTS)
            un = R.units(tr["f0"], tr["tau"], en, d[i], S, None if g is None else g[i])
            sl = slice(off[i], off[i + 1])
            assert np.array_equal(out["energy_frames"]["energy"].cpu().numpy()[sl], en)
            assert np.array_equal(out["track"]["tau"].cpu().numpy()[sl], tr["tau"])
            assert np.array_equal(bits(out["track"]["f0"].cpu().numpy()[sl]), bits(tr["f0"]))
            assert bits(out["track"]["score"].cpu().numpy()[i]) == bits(tr["score"])
            got = {k: out[k].cpu().numpy()[i] for k in prosody.UNIT_SUMS}
            got.update(cont=out["cont"].cpu().numpy()[sl], units=int(out["units"].cpu()[i]), status=int(out["status"].cpu()[i]))
            same_units(got, un)
            for k, v in R.means(un).items():
                assert np.array_equal(bits(out[k].cpu().numpy()[i]), bits(v)), k
            voiced_total += int((tr["tau"] > 0).sum())
        assert voiced_total > 0


def test_prosody_targets_vocoded_shapes_and_repeatability(default_hp):
    from b2s_hip import prosody
    hp = default_hp
    rng = np.random.default_rng(4)
    frames, S = [12, 9, 1], 4
    mels = np.clip(rng.standard_normal((3, 12, int(hp.num_mels))), -4, 4).astype(np.float32)
    d = np.zeros((3, S), np.int32)
    d[0], d[1], d[2, :1] = dur_ref.random_durations(rng, S, 12), dur_ref.random_durations(rng, S, 9), [1]
    a = prosody.prosody_targets(mels, frames, d, [S, S, 1], n_iter=2, hp=hp)
    b = prosody.prosody_targets(torch.from_numpy(mels).to(DEV), frames, d, [S, S, 1], n_iter=2, hp=hp)
    assert a["track"]["frames"] == frames and a["cont"].shape == (sum(frames),)
    assert all(a[k].shape == (3, S) for k in prosody.UNIT_SUMS + prosody.TARGETS)
    assert a["frames"].sum(dim=1).cpu().tolist() == frames and a["units"].cpu().tolist() == [S, S, 1]
    assert set(a["status"].cpu().tolist()) <= {R.OK, R.NOVOICE}
    for k in ("cont", "pitch", "pitch_voiced", "energy", "f0_voiced_sum", "f0_cont_sum"):
        assert torch.equal(a[k].view(torch.int64), b[k].view(torch.int64)), k
    for k in ("frames", "voiced", "energy_sum", "units", "status"):
        assert torch.equal(a[k], b[k]), k


def test_command_line_extracts_prosody_targets(tmp_path, capsys):
    import hyperparams
    from hyperparams import hparams as hp
    from b2s_hip import prosody
    from oracle import synth, make_config, TINY96
    from transformer.tacotron import Tacotron
    from utils.checkpoint import save_model
    from utils.text import text_to_byte_sequence
    hp.override_from_dict(hyperparams.DEFAULTS)
    hp.parse(TINY96)
    hp.parse("compute_dtype=fp32,max_generation_frames=40")
    try:
        st = synth.synthetic_state(make_config(TINY96), 1234)
        m = Tacotron(hp)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in st.items()})
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
            assert prosody.main([ckpt, "--data-dir", str(data), "--out", str(out), "--batch", "2", "--units", units, "--n-iter", "2"]) == 0
            printed = json.loads(capsys.readouterr().out)
            assert printed["utterances"] == 3 and printed["written"] == 3 and printed["units"] == units
            recs = [json.loads(line) for line in open(out / "prosody.jsonl", encoding="utf-8")]
            assert [r["name"] for r in recs] == names
            n_units = 0
            for r, n, text, t in zip(recs, names, texts, frames):
                z = np.load(out / (n + ".npz"))
                want_units = len(text_to_byte_sequence(text)) if units == "bytes" else len(text) + 2
                assert sorted(z.files) == ["duration", "energy", "pitch", "pitch_voiced", "voiced_frames"]
                assert all(z[k].shape == (want_units,) for k in z.files)
                assert z["duration"].dtype == np.int32 and int(z["duration"].sum()) == t and z["duration"].min() >= 1
                assert np.all(z["voiced_frames"] <= z["duration"]) and np.all(z["energy"] >= 0) and np.all(z["pitch"] >= 0)
                assert r["status"] in ("OK", "NOVOICE") and r["frames"] == t and r["units"] == want_units
                assert 0.0 <= r["voiced_share"] <= 1.0 and abs(r["voiced_share"] - z["voiced_frames"].sum() / t) < 1e-12
                n_units += want_units
            assert not (out / "spkA_0004.npz").exists()
            stats = json.load(open(out / "stats.json", encoding="utf-8"))
            assert stats["units"] == units and stats["utterances"] == 3
            assert stats["overall"]["pitch"]["count"] == stats["overall"]["energy"]["count"] == n_units
            assert sorted(stats["languages"]) == ["de-de", "en-us"]
            assert sum(v["energy"]["count"] for v in stats["languages"].values()) == n_units
    finally:
        hp.override_from_dict(hyperparams.DEFAULTS)
