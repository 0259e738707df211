"""GPU tests of the YIN pitch tracker and the F0 error after DTW (b2s_hip.f0, libb2s_f0.so) against the NumPy restatement
tests/f0_ref.py.

One batch of 9 utterances with lengths {0, 2, 199, 200, 201, 1066, 1067, 2400, 4000}: at the default parameters a segment is 1066
samples, so frames leave the signal at one end, at both ends and at neither.  Gates: the PCM, tau and status are EQUAL to the
oracle's; cmnd, aper and f0 are bit-equal (compared as int64): every sum of the estimator is an exact integer, the one division and
the refinement are single fp64 operations.  The counts and the ratios of the score are EQUAL, its two RMSEs are within 1e-12
relative (at most ~2100 summed terms: the fp64 bound is under 3e-13, log2 adds a few ulp)."""
import json
import types
import zipfile

import numpy as np
import pytest
import torch

import f0_ref as R

pytestmark = pytest.mark.gpu

LENGTHS = [0, 2, 199, 200, 201, 1066, 1067, 2400, 4000]
# win, hop, tau_min, tau_max
PARAMS = [(800, 200, 32, 266), (64, 16, 2, 32), (2048, 200, 2, 512), (801, 199, 33, 265)]
SR, THRESHOLD = 16000.0, 0.1
RTOL = 1e-12
SENTINEL = -12345.0
HP = types.SimpleNamespace(sr=16000, win_length=800, hop_length=200)
# which content has which of LENGTHS, in the two assignments
ORDER = [["zeros", "constant", "noise", "40hz", "700hz", "tone_noise", "square", "sine100", "octave"],
         ["constant", "zeros", "sine100", "octave", "square", "noise", "40hz", "tone_noise", "700hz"]]


def ids(p):
    return "win%d-hop%d-tau%d..%d" % p


def make_waves(variant=0):
    """The 9 utterances, fp32, in the order of LENGTHS.  Nine contents meet nine lengths, of which four hold a whole segment; so there
    are two assignments, and every content that needs room to show what it is there for gets it in one of them."""
    rng = np.random.default_rng(20260101 + variant)

    def octave(L):
        n = np.arange(L)
        w = 0.5 * np.sin(2 * np.pi * 130.81 / SR * n) + 0.3 * np.sin(2 * np.pi * 261.62 / SR * n)
        w[L * 7 // 10:] *= 0.003                                     # a tail about 50 dB down: what silence_db switches off
        return w

    def tone_noise(L):
        w = np.sin(2 * np.pi * 200.0 / SR * np.arange(L)) + 0.2 * rng.standard_normal(L)
        return w * (3.7 / max(np.abs(w).max(), 1e-9)) if L else w    # peak 3.7: the peak normalisation
    contents = {"zeros": lambda L: np.zeros(L),
                "constant": lambda L: np.full(L, 0.25),
                "noise": lambda L: rng.standard_normal(L),                                  # no voiced frame
                "40hz": lambda L: 0.8 * np.sin(2 * np.pi * 40.0 / SR * np.arange(L)),       # below fmin: unvoiced
                "700hz": lambda L: 0.8 * np.sin(2 * np.pi * 700.0 / SR * np.arange(L)),     # above fmax: picked an octave below
                "tone_noise": tone_noise,
                "square": lambda L: np.where((np.arange(L) / 123.4) % 1.0 < 0.5, 1.0, -1.0),    # full scale: the largest d
                "sine100": lambda L: 0.7 * np.sin(2 * np.pi * np.arange(L) / 100.0),        # integer period 100
                "octave": octave}                                                          # 130.81 Hz plus its octave
    waves = [contents[name](L).astype(np.float32) for name, L in zip(ORDER[variant], LENGTHS)]
    assert [len(w) for w in waves] == LENGTHS
    return waves


def padded(rows, dtype):
    out = np.zeros((len(rows), max(max(len(r) for r in rows), 1)), dtype)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


_cache = {}


def batch(variant=0):
    """Waves, their oracle PCM (computed once and left unchanged)."""
    if ("batch", variant) not in _cache:
        waves = make_waves(variant)
        _cache["batch", variant] = (waves, [R.quantize(w)[0] for w in waves])
    return _cache["batch", variant]


def run_yin(pcm_rows, lengths, prm, floor=0, offsets=None, guard=3):
    """b2s_f0_yin through the C ABI on a padded int16 batch, with `guard` sentinel rows behind every output; they must stay
    untouched.  Returns host arrays."""
    from b2s_hip import f0
    l = f0.load()
    dev = torch.device("cuda")
    win, hop, tau_min, tau_max = prm
    B = len(pcm_rows)
    pcm = torch.from_numpy(padded(pcm_rows, np.int16)).to(dev)
    Lmax = int(pcm.shape[1])
    frames = [1 + len(r) // hop for r in pcm_rows]                            # the true ones, whatever `lengths` claims
    off = np.concatenate([[0], np.cumsum(frames)]).astype(np.int32) if offsets is None else np.asarray(offsets, np.int32)
    total = int(np.sum(frames))
    out_f0 = torch.full((total + guard,), SENTINEL, dtype=torch.float64, device=dev)
    out_tau = torch.full((total + guard,), -7, dtype=torch.int32, device=dev)
    out_aper = torch.full((total + guard,), SENTINEL, dtype=torch.float64, device=dev)
    out_c = torch.full((total + guard, tau_max + 1), SENTINEL, dtype=torch.float64, device=dev)
    status = torch.full((B + guard,), -7, dtype=torch.int32, device=dev)
    lens = torch.tensor(lengths, dtype=torch.int32, device=dev)
    off_d = torch.from_numpy(off).to(dev)
    f0.check(l.b2s_f0_yin(pcm.data_ptr(), lens.data_ptr(), off_d.data_ptr(), total, B, Lmax, win, hop, tau_min, tau_max, THRESHOLD,
                          int(floor), SR, out_f0.data_ptr(), out_tau.data_ptr(), out_aper.data_ptr(), out_c.data_ptr(),
                          status.data_ptr(), None))
    torch.cuda.synchronize()
    res = {"f0": out_f0.cpu().numpy(), "tau": out_tau.cpu().numpy(), "aper": out_aper.cpu().numpy(), "cmnd": out_c.cpu().numpy(),
           "status": status.cpu().numpy(), "offsets": off, "total": total}
    assert np.all(res["f0"][total:] == SENTINEL) and np.all(res["tau"][total:] == -7) and np.all(res["aper"][total:] == SENTINEL)
    assert np.all(res["cmnd"][total:] == SENTINEL) and np.all(res["status"][B:] == -7)
    for k in ("f0", "tau", "aper", "cmnd"):
        res[k] = res[k][:total]
    res["status"] = res["status"][:B]
    return res


def case(prm, floor=0, variant=0):
    key = (prm, floor, variant)
    if key not in _cache:
        waves, pcms = batch(variant)
        win, hop, tau_min, tau_max = prm
        ref = [R.yin(p, win, hop, tau_min, tau_max, THRESHOLD, floor, SR) for p in pcms]
        _cache[key] = (ref, run_yin(pcms, LENGTHS, prm, floor))
    return _cache[key]


def assert_equal_to_oracle(got, ref, what=""):
    for k in ("cmnd", "aper", "f0"):
        want = np.concatenate([r[k] for r in ref])
        assert got[k].shape == want.shape and got[k].dtype == np.float64
        diff = got[k].view(np.int64) != want.view(np.int64)
        print("%s %s: %d of %d fp64 values differ" % (what, k, diff.sum(), diff.size))
        assert not diff.any(), "%s %s: %d of %d differ, first at %s: %r vs %r" % (
            what, k, diff.sum(), diff.size, np.argwhere(diff)[0], got[k][diff][0], want[diff][0])
    assert np.array_equal(got["tau"], np.concatenate([r["tau"] for r in ref]))


# ------------------------------------------------------------------------------------------------------------------ quantise

def test_quantised_pcm_peak_and_status_equal_the_oracle():
    from b2s_hip import f0
    waves, pcms = batch()
    out = f0.quantize_batch(padded(waves, np.float32), LENGTHS)
    pcm, peak, status = out["pcm"].cpu().numpy(), out["peak"].cpu().numpy(), out["status"].cpu().numpy()
    assert pcm.dtype == np.int16 and pcm.shape == (9, 4000) and status.tolist() == [f0.OK] * 9
    for b, want in enumerate(pcms):
        assert np.array_equal(pcm[b, :LENGTHS[b]], want) and np.all(pcm[b, LENGTHS[b]:] == 0)
        assert peak[b] == (np.abs(waves[b]).max() if LENGTHS[b] else 0)
    assert abs(peak[5] - 3.7) < 1e-6 and np.abs(pcms[5]).max() == 32767 and np.abs(pcms[7]).max() == 32767
    ragged = f0.quantize_batch(waves)                                         # a list of 1-D arrays carries its own lengths
    assert ragged["lengths"] == LENGTHS and torch.equal(ragged["pcm"], out["pcm"])


def test_a_nan_and_an_inf_fail_their_own_utterance():
    from b2s_hip import f0
    waves, pcms = batch()
    rows = [waves[7].copy(), waves[8].copy(), waves[6].copy(), waves[5].copy()]
    rows[1][3999] = np.nan                                                    # the last sample
    rows[2][0] = np.inf
    rows[3] = np.concatenate([rows[3], [np.nan]]).astype(np.float32)          # a NaN behind the length is not looked at
    out = f0.quantize_batch(padded(rows, np.float32), [2400, 4000, 1067, 1066])
    pcm, status = out["pcm"].cpu().numpy(), out["status"].cpu().numpy()
    assert status.tolist() == [f0.OK, f0.FAILED, f0.FAILED, f0.OK]
    assert np.array_equal(pcm[0, :2400], pcms[7]) and np.array_equal(pcm[3, :1066], pcms[5])
    assert not pcm[1].any() and not pcm[2].any() and not pcm[3, 1066:].any()
    assert out["peak"].cpu().numpy()[1:3].tolist() == [0, 0]
    y = f0.yin_batch(padded(rows, np.float32), [2400, 4000, 1067, 1066], hp=HP)      # the failure is handed on
    assert y["status"].cpu().tolist() == [f0.OK, f0.FAILED, f0.FAILED, f0.OK]
    with pytest.raises(f0.B2SError, match="NaN or Inf"):
        f0.f0(rows[1], hp=HP)


# ----------------------------------------------------------------------------------------------------------------------- YIN

@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("prm", PARAMS, ids=ids)
def test_yin_is_bit_equal_to_the_oracle(prm, variant):
    from b2s_hip import f0
    ref, got = case(prm, 0, variant)
    assert got["status"].tolist() == [f0.OK] * 9
    assert got["offsets"].tolist() == [0] + np.cumsum([1 + n // prm[1] for n in LENGTHS]).tolist()
    assert_equal_to_oracle(got, ref, ids(prm))
    assert np.all((got["f0"] > 0) == (got["tau"] > 0))


def test_what_the_contents_are_there_for():
    """At the default parameters, frames whose segment lies inside the signal: the sine of period 100 is picked at 100, the two
    tones at the period of the lower one, and the largest d of the square wave is past what fp32 or int32 can hold exactly."""
    ref, got = case(PARAMS[0])
    o = got["offsets"]
    sine, octave = got["tau"][o[7]:o[8]], got["tau"][o[8]:o[9]]
    assert sine[3:10].tolist() == [100] * 7
    assert np.all(np.abs(got["f0"][o[8]:o[9]][3:11] - 130.81) < 1.0) and octave[3:11].tolist() == [122] * 8
    waves, pcms = batch()
    d = R.difference(R.segment(pcms[6], 3, 800, 200, 266), 800, 266)
    assert int(d.max()) > 2 ** 40 and got["tau"][o[6] + 3] in (123, 124)
    # the other assignment: noise and 40 Hz have no voiced frame, 700 Hz (period 22.9 < tau_min) is picked at two periods
    ref, got = case(PARAMS[0], 0, 1)
    o = got["offsets"]
    assert ORDER[1][5:] == ["noise", "40hz", "tone_noise", "700hz"]
    assert not got["tau"][o[5]:o[7]].any() and got["tau"][o[7]:o[8]].any()
    assert np.all(got["tau"][o[8]:o[9]] == 46) and np.all(np.abs(got["f0"][o[8]:o[9]] - 350.0) < 1.0)


@pytest.mark.parametrize("prm", [PARAMS[0], PARAMS[3]], ids=ids)
def test_bits_repeat_and_do_not_depend_on_the_batch(prm):
    ref, got = case(prm)
    waves, pcms = batch()
    again = run_yin(pcms, LENGTHS, prm)
    for k in ("f0", "tau", "aper", "cmnd"):
        assert np.array_equal(again[k].view(np.uint8), got[k].view(np.uint8)), k
    o = got["offsets"]
    for b in (0, 4, 6, 8):                                                    # B = 1, L = 0 among them
        alone = run_yin([pcms[b]], [LENGTHS[b]], prm)
        assert alone["status"].tolist() == [0]
        for k in ("f0", "tau", "aper", "cmnd"):
            assert np.array_equal(alone[k].view(np.uint8), got[k][o[b]:o[b + 1]].view(np.uint8)), (b, k)
    pair = run_yin([pcms[8], pcms[5]], [4000, 1066], prm)                     # another batch, another order
    for k in ("f0", "tau", "aper", "cmnd"):
        want = np.concatenate([got[k][o[8]:o[9]], got[k][o[5]:o[6]]])
        assert np.array_equal(pair[k].view(np.uint8), want.view(np.uint8)), k


def test_python_binding_gives_the_bits_of_the_c_abi():
    from b2s_hip import f0
    prm = PARAMS[0]
    ref, got = case(prm)
    waves, pcms = batch()
    kw = dict(win=prm[0], hop=prm[1], tau_min=prm[2], tau_max=prm[3], threshold=THRESHOLD, silence_db=None, sr=SR)
    for source in (padded(waves, np.float32), torch.from_numpy(padded(pcms, np.int16)).cuda()):
        y = f0.yin_batch(source, LENGTHS, return_cmnd=True, **kw)
        assert y["frame_offsets"].tolist() == got["offsets"].tolist() and y["frames"] == np.diff(got["offsets"]).tolist()
        assert y["status"].cpu().tolist() == [f0.OK] * 9
        for k in ("f0", "tau", "aper", "cmnd"):
            assert np.array_equal(y[k].cpu().numpy().view(np.uint8), got[k].view(np.uint8)), k
    one = f0.f0(waves[7], hp=HP, silence_db=None)
    o = got["offsets"]
    assert one.dtype == np.float64 and np.array_equal(one.view(np.int64), got["f0"][o[7]:o[8]].view(np.int64))


def test_silence_floor_switches_frames_off_where_the_integer_comparison_does():
    prm = PARAMS[0]
    ref0, got0 = case(prm)
    floor = R.min_energy(prm[0], -40)
    ref, got = case(prm, floor)
    assert_equal_to_oracle(got, ref, "silence -40 dB")
    off = (got0["tau"] > 0) & (got["tau"] == 0)
    assert off.any() and (got["tau"] > 0).any()
    assert np.array_equal(got["cmnd"].view(np.int64), got0["cmnd"].view(np.int64))           # the floor touches the pick only
    # exactly at a frame's own energy: e keeps it, e + 1 switches it off
    o = got0["offsets"]
    t = 5
    e = ref0[7]["energy"][t]
    assert got0["tau"][o[7] + t] == 100
    waves, pcms = batch()
    assert run_yin([pcms[7]], [2400], prm, floor=e)["tau"][t] == 100
    assert run_yin([pcms[7]], [2400], prm, floor=e + 1)["tau"][t] == 0


def test_a_bad_length_or_offsets_fail_that_utterance_alone():
    from b2s_hip import f0
    prm = PARAMS[0]
    ref, got = case(prm)
    waves, pcms = batch()
    o = got["offsets"].copy()
    # utterance 3 claims a frame too many, utterance 5 starts below 0; the others keep their rows
    bad = o.copy()
    bad[4] += 1
    res = run_yin(pcms, LENGTHS, prm, offsets=bad)
    assert res["status"].tolist() == [0, 0, 0, f0.FAILED, f0.FAILED, 0, 0, 0, 0]
    for b in range(9):
        rows = slice(o[b], o[b + 1])
        if b in (3, 4):
            assert np.all(res["f0"][rows] == SENTINEL) and np.all(res["tau"][rows] == -7) and np.all(res["cmnd"][rows] == SENTINEL)
        else:
            for k in ("f0", "tau", "aper", "cmnd"):
                assert np.array_equal(res[k][rows].view(np.uint8), got[k][rows].view(np.uint8)), (b, k)
    neg = o.copy()
    neg[0] = -1
    assert run_yin(pcms, LENGTHS, prm, offsets=neg)["status"].tolist() == [f0.FAILED] + [0] * 8
    past = o.copy()
    past[9] += 200                                                            # the last utterance runs past total_frames
    assert run_yin(pcms, LENGTHS, prm, offsets=past)["status"].tolist() == [0] * 8 + [f0.FAILED]
    # lengths outside 0..Lmax: nothing of that utterance is read or written
    for wrong in (-1, 4001, 2 ** 31 - 1):
        lengths = list(LENGTHS)
        lengths[7] = wrong
        res = run_yin(pcms, lengths, prm, offsets=o)
        assert res["status"].tolist() == [0] * 7 + [f0.FAILED, 0]
        assert np.all(res["f0"][o[7]:o[8]] == SENTINEL)
        assert np.array_equal(res["f0"][o[8]:o[9]].view(np.int64), got["f0"][o[8]:o[9]].view(np.int64))


# --------------------------------------------------------------------------------------------------------------------- score

def run_score(tracks_x, tracks_y, kept_x, kept_y, paths, dtw_status=None, path_len=None, gross_ratio=0.2, slack=2):
    """b2s_f0_score through the C ABI on hand-built data: tracks = list of (f0, tau), kept = list of int lists, paths = list of
    (i, j) lists; every path slot has `slack` unused pairs behind it."""
    from b2s_hip import f0
    l = f0.load()
    dev = torch.device("cuda")
    B = len(paths)

    def pack(rows, dtype):
        flat = np.concatenate([np.asarray(r, dtype).reshape(-1) for r in rows] + [np.zeros(0, dtype)])
        off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
        return torch.from_numpy(flat).to(dev), torch.from_numpy(off).to(dev), int(off[-1])
    fx, fxo, tfx = pack([t[0] for t in tracks_x], np.float64)
    tx = pack([t[1] for t in tracks_x], np.int32)[0]
    fy, fyo, tfy = pack([t[0] for t in tracks_y], np.float64)
    ty = pack([t[1] for t in tracks_y], np.int32)[0]
    kx, kxo, tkx = pack(kept_x, np.int32)
    ky, kyo, tky = pack(kept_y, np.int32)
    slots = [list(p) + [(-9, -9)] * slack for p in paths]
    path = torch.from_numpy(np.concatenate([np.asarray(s, np.int32).reshape(-1, 2) for s in slots])).to(dev)
    po = torch.from_numpy(np.concatenate([[0], np.cumsum([len(s) for s in slots])]).astype(np.int32)).to(dev)
    plen = torch.tensor([len(p) for p in paths] if path_len is None else path_len, dtype=torch.int32, device=dev)
    dstat = torch.tensor([0] * B if dtw_status is None else dtw_status, dtype=torch.int32, device=dev)
    scores = torch.full((B + 1, 5), SENTINEL, dtype=torch.float64, device=dev)
    counts = torch.full((B + 1, 4), -7, dtype=torch.int32, device=dev)
    status = torch.full((B + 1,), -7, dtype=torch.int32, device=dev)
    f0.check(l.b2s_f0_score(fx.data_ptr(), tx.data_ptr(), fxo.data_ptr(), tfx, fy.data_ptr(), ty.data_ptr(), fyo.data_ptr(), tfy,
                            kx.data_ptr(), kxo.data_ptr(), tkx, ky.data_ptr(), kyo.data_ptr(), tky, B, path.data_ptr(), po.data_ptr(),
                            int(path.shape[0]), plen.data_ptr(), dstat.data_ptr(), gross_ratio, scores.data_ptr(), counts.data_ptr(),
                            status.data_ptr(), None))
    torch.cuda.synchronize()
    s, c, st = scores.cpu().numpy(), counts.cpu().numpy(), status.cpu().numpy()
    assert np.all(s[B] == SENTINEL) and np.all(c[B] == -7) and st[B] == -7
    return s[:B], c[:B], st[:B]


def assert_score(got_s, got_c, got_st, want):
    assert int(got_st) == want["status"] and got_c.tolist() == want["counts"]
    for k in (2, 3, 4):                                                       # vde, gpe, ffe: EQUAL
        assert (np.isnan(got_s[k]) and np.isnan(want["scores"][k])) or got_s[k] == want["scores"][k], k
    for k in (0, 1):
        if np.isnan(want["scores"][k]):
            assert np.isnan(got_s[k])
        else:
            print("score %d: %.15g vs %.15g" % (k, got_s[k], want["scores"][k]))
            assert want["scores"][k] > 0 and abs(got_s[k] - want["scores"][k]) <= RTOL * want["scores"][k]


def hand_built():
    """5 pairs: a long random one (2100 steps: several rounds of the 256 threads), a short one, one without a common voiced step,
    one with an empty path, one whose kept maps skip frames."""
    rng = np.random.default_rng(11)

    def track(F, p_unvoiced):
        f = rng.uniform(70.0, 400.0, F)
        tau = np.rint(SR / f).astype(np.int32)
        dead = rng.uniform(size=F) < p_unvoiced
        f[dead], tau[dead] = 0.0, 0
        return f, tau

    def walk_path(nx, ny, steps):
        i = np.minimum(np.arange(steps) * nx // steps, nx - 1)
        j = np.minimum((np.arange(steps) * ny + ny // 2) // steps, ny - 1)
        return list(zip(i.tolist(), j.tolist()))
    tx = [track(1500, 0.3), track(7, 0.0), track(40, 0.0), track(9, 0.2), track(300, 0.3)]
    ty = [track(1400, 0.3), track(5, 0.0), track(30, 0.0), track(9, 0.2), track(280, 0.3)]
    tx[2][0][:20], tx[2][1][:20] = 0.0, 0                                     # x voiced only in its second half,
    ty[2][0][10:], ty[2][1][10:] = 0.0, 0                                     # y only at its start
    kept_x = [np.arange(1500), np.arange(7), np.arange(40), np.arange(9), np.sort(rng.choice(300, 200, replace=False))]
    kept_y = [np.arange(1400), np.arange(5), np.arange(30), np.arange(9), np.sort(rng.choice(280, 190, replace=False))]
    paths = [walk_path(1500, 1400, 2100), walk_path(7, 5, 9), [(i, i * 30 // 40) for i in range(20, 40)], [],
             walk_path(200, 190, 333)]
    return tx, ty, kept_x, kept_y, paths


def test_score_counts_and_ratios_equal_the_oracle_and_the_rmse_is_within_1e_12():
    from b2s_hip import f0
    tx, ty, kept_x, kept_y, paths = hand_built()
    s, c, st = run_score(tx, ty, kept_x, kept_y, paths)
    want = [R.score(tx[b][0], tx[b][1], ty[b][0], ty[b][1], kept_x[b], kept_y[b], paths[b]) for b in range(5)]
    assert st.tolist() == [f0.OK, f0.OK, f0.OK, f0.EMPTY, f0.OK]
    for b in range(5):
        assert_score(s[b], c[b], st[b], want[b])
    assert c[0, 0] == 2100 and c[0, 2] > 500 and c[0, 3] > 0 and c[0, 1] > 0
    assert c[2].tolist() == [20, 20, 0, 0] and np.isnan(s[2, 0]) and np.isnan(s[2, 1]) and np.isnan(s[2, 3]) and s[2, 2] == 1.0
    assert np.all(np.isnan(s[3])) and c[3].tolist() == [0, 0, 0, 0]
    # the same bits on a second call, and for a pair alone
    s2, c2, st2 = run_score(tx, ty, kept_x, kept_y, paths)
    assert np.array_equal(s2.view(np.int64), s.view(np.int64)) and np.array_equal(c2, c)
    for b in (0, 4):
        s1, c1, st1 = run_score(tx[b:b + 1], ty[b:b + 1], kept_x[b:b + 1], kept_y[b:b + 1], paths[b:b + 1])
        assert np.array_equal(s1[0].view(np.int64), s[b].view(np.int64)) and np.array_equal(c1[0], c[b])
    # another gross ratio moves the gross count only
    s3, c3, st3 = run_score(tx, ty, kept_x, kept_y, paths, gross_ratio=0.05)
    want3 = R.score(tx[0][0], tx[0][1], ty[0][0], ty[0][1], kept_x[0], kept_y[0], paths[0], gross_ratio=0.05)
    assert_score(s3[0], c3[0], st3[0], want3)
    assert c3[0, 3] > c[0, 3] and c3[0, :3].tolist() == c[0, :3].tolist()


def test_out_of_range_indices_fail_that_pair_only():
    from b2s_hip import f0
    tx, ty, kept_x, kept_y, paths = hand_built()
    s, c, st = run_score(tx, ty, kept_x, kept_y, paths)

    def others_unchanged(s2, c2, st2, failed):
        for b in range(5):
            if b == failed:
                assert st2[b] == f0.FAILED and np.all(np.isnan(s2[b])) and c2[b].tolist() == [0, 0, 0, 0]
            else:
                assert st2[b] == st[b] and np.array_equal(s2[b].view(np.int64), s[b].view(np.int64)) and np.array_equal(c2[b], c[b])
    for wrong in ((7, 0), (-1, 0), (0, 5), (0, -2), (2 ** 31 - 1, 0)):        # a path index outside the kept count
        p = [list(q) for q in paths]
        p[1][4] = wrong
        others_unchanged(*run_score(tx, ty, kept_x, kept_y, p), failed=1)
    for side, wrong in ((0, 300), (0, -1), (1, 280), (1, 2 ** 31 - 1)):       # a frame number outside the F0 track
        kx, ky = [k.copy() for k in kept_x], [k.copy() for k in kept_y]
        (kx, ky)[side][4][100] = wrong
        others_unchanged(*run_score(tx, ty, kx, ky, paths), failed=4)
    # the DTW's statuses are handed on; a path_len past its slot is refused
    s2, c2, st2 = run_score(tx, ty, kept_x, kept_y, paths, dtw_status=[0, f0.EMPTY, f0.FAILED, 0, 0])
    assert st2.tolist() == [f0.OK, f0.EMPTY, f0.FAILED, f0.EMPTY, f0.OK] and np.all(np.isnan(s2[1:4])) and not c2[1:4].any()
    others_unchanged(*run_score(tx, ty, kept_x, kept_y, paths, path_len=[2100, 9 + 3, 20, 0, 333]), failed=1)
    others_unchanged(*run_score(tx, ty, kept_x, kept_y, paths, path_len=[2100, -1, 20, 0, 333]), failed=1)


# ---------------------------------------------------------------------------------------------------------------- end to end

def walk(rng, T, n_mels=80, lim=4.0):
    return np.clip(np.cumsum(rng.standard_normal((T, n_mels)) * 0.3, axis=0), -lim, lim).astype(np.float32)


def hp_of():
    import hyperparams
    hp = hyperparams.hparams
    hp.override_from_dict(hyperparams.DEFAULTS)
    return hp


def test_f0_after_dtw_end_to_end_against_the_oracle_on_the_returned_pcm_and_path():
    from b2s_hip import f0
    hp = hp_of()
    rng = np.random.default_rng(8)
    LX, LY = [20, 45, 70, 33], [28, 70, 61, 30]
    xs, ys = [walk(rng, n) for n in LX], [walk(rng, n) for n in LY]
    xs[2][10:14] = -4.0                                                       # frames that are not kept
    ys[1][0:2] = -4.0
    ys[3][:] = -4.0                                                           # pair 3: no kept frame on the target side
    preds, targets = np.zeros((4, 70, 80), np.float32), np.zeros((4, 70, 80), np.float32)
    for b in range(4):
        preds[b, :LX[b]], targets[b, :LY[b]] = xs[b], ys[b]
    kw = dict(threshold=0.3, silence_db=-60.0)        # random-walk mels vocode to noise-like audio: a loose threshold voices some frames
    out = f0.f0_dtw_details(preds, LX, targets, LY, n_iter=4, hp=hp, **kw)
    status = out["status"].cpu().numpy()
    assert status.tolist() == [f0.OK, f0.OK, f0.OK, f0.EMPTY]
    prm = out["x"]["params"]
    assert (prm["win"], prm["hop"], prm["tau_min"], prm["tau_max"], prm["min_energy"]) == (800, 200, 32, 266, R.min_energy(800, -60.0))
    path, po, plen = out["path"].cpu().numpy(), out["path_offsets"], out["path_len"].cpu().numpy()
    scores, counts = out["scores"].cpu().numpy(), out["counts"].cpu().numpy()
    tracks = {}
    for side, mels, lens in (("x", xs, LX), ("y", ys, LY)):
        y = out[side]
        pcm, fo = y["pcm"].cpu().numpy(), y["frame_offsets"]
        assert y["lengths"] == [200 * (n - 1) for n in lens] and y["frames"] == lens and y["status"].cpu().tolist() == [0] * 4
        ref = [R.yin(pcm[b, :y["lengths"][b]], 800, 200, 32, 266, 0.3, prm["min_energy"], 16000.0) for b in range(4)]
        got = {k: y[k].cpu().numpy() for k in ("f0", "tau", "aper")}
        for k in ("f0", "aper"):
            assert np.array_equal(got[k].view(np.int64), np.concatenate([r[k] for r in ref]).view(np.int64)), (side, k)
        assert np.array_equal(got["tau"], np.concatenate([r["tau"] for r in ref]))
        assert np.abs(pcm).max() == 32767
        kept, ko = out["kept_" + side].cpu().numpy(), out["kept_offsets_" + side].cpu().numpy()
        for b in range(4):
            assert kept[ko[b]:ko[b + 1]].tolist() == np.nonzero(mels[b].max(axis=1) > 0)[0].tolist()
        tracks[side] = (ref, kept, ko)
    for b in range(4):
        (rx, kx, kxo), (ry, ky, kyo) = tracks["x"], tracks["y"]
        want = R.score(rx[b]["f0"], rx[b]["tau"], ry[b]["f0"], ry[b]["tau"], kx[kxo[b]:kxo[b + 1]], ky[kyo[b]:kyo[b + 1]],
                       path[po[b]:po[b] + plen[b]])
        if b == 3:
            assert want["status"] == R.EMPTY and np.all(np.isnan(scores[b])) and not counts[b].any()
            continue
        assert plen[b] >= max(kxo[b + 1] - kxo[b], kyo[b + 1] - kyo[b])
        assert_score(scores[b], counts[b], status[b], want)
    print("end to end: counts", counts.tolist())
    for i, k in enumerate(f0.SCORES):
        assert torch.equal(out[k], out["scores"][:, i])
    # the dict and list functions, an empty batch, a one-frame utterance on a vocoded side
    res = f0.f0_dtw_batch(preds, LX, targets, LY, n_iter=4, hp=hp, **kw)
    assert sorted(res) == sorted(f0.SCORES + f0.COUNTS + ("status",))
    assert np.array_equal(res["rmse_hz"].cpu().numpy().view(np.int64), scores[:, 0].view(np.int64))
    recs = f0.calculate_f0_dtw(preds, LX, targets, LY, n_iter=4, hp=hp, **kw)
    assert recs[3] is None and [r["steps"] for r in recs[:3]] == counts[:3, 0].tolist() and type(recs[0]["vde"]) is float
    empty = f0.f0_dtw_batch(preds[:0], [], targets[:0], [], hp=hp)
    assert empty["ffe"].shape == (0,) and empty["ffe"].dtype == torch.float64 and empty["steps"].dtype == torch.int32
    assert f0.calculate_f0_dtw(preds[:0], [], targets[:0], []) == []
    short = f0.f0_dtw_details(preds[:2], [1, 45], targets[:2], LY[:2], n_iter=4, hp=hp, **kw)
    assert short["status"].cpu().tolist() == [f0.EMPTY, f0.OK] and short["steps"].cpu().tolist()[0] == 0
    assert short["steps"].cpu().tolist()[1] == counts[1, 0] and short["x"]["lengths"] == [0, 200 * 44]
    # waveforms handed in: a NaN fails its pair and raises in the batch call
    wavs = [out["x"]["pcm"][b, :out["x"]["lengths"][b]].float().cpu().numpy() / 32767 for b in range(4)]
    given = f0.f0_dtw_details(preds, LX, targets, LY, pred_wavs=wavs, n_iter=4, hp=hp, **kw)
    assert torch.equal(given["x"]["pcm"], out["x"]["pcm"]) and torch.equal(given["counts"], out["counts"])
    wavs[1][5] = np.nan
    assert f0.f0_dtw_details(preds, LX, targets, LY, pred_wavs=wavs, n_iter=4, hp=hp, **kw)["status"].cpu().tolist() == \
        [f0.OK, f0.FAILED, f0.OK, f0.EMPTY]
    with pytest.raises(f0.B2SError, match=r"failed for pairs \[1\]"):
        f0.f0_dtw_batch(preds, LX, targets, LY, pred_wavs=wavs, n_iter=4, hp=hp, **kw)


def test_command_line_rescoring_of_a_finished_eval(tmp_path, capsys):
    from b2s_hip import f0, rescore
    hp = hp_of()
    rng = np.random.default_rng(5)
    names = ["spk1_%02d" % i for i in range(6)]
    langs = ["en-us", "de-de", "en-us", "de-de", "en-us", "en-us"]
    truth = [walk(rng, int(n)) for n in (40, 55, 64, 70, 33, 20)]
    truth[5][:] = -4.0                                               # a target with no kept frame: counted as empty
    data, ev = tmp_path / "data", tmp_path / "eval_10"
    data.mkdir()
    ev.mkdir()
    with zipfile.ZipFile(data / "mels.zip", "w") as z:
        for n, m in zip(names, truth):
            with z.open(n + ".npy", "w") as f:
                np.save(f, m)
    (data / "metadata.eval.txt").write_text("".join("%s.npy|%d|text %s|%s\n" % (n, len(m), n, l)
                                                    for n, m, l in zip(names, truth, langs)), encoding="utf-8")
    gen = [np.clip(m[::2].repeat(2, axis=0)[:len(m) - 3] + 0.2 * rng.standard_normal((len(m) - 3, 80)), -4, 4).astype(np.float32)
           for m in truth]
    for n, g in zip(names, gen):
        np.save(ev / (n + ".npy"), g)
    np.save(ev / "spk9_99.npy", gen[0])                              # generated, but not in mels.zip
    out = tmp_path / "f0.json"
    args = ["--batch", "4", "--n-iter", "4", "--threshold", "0.3", "--silence-db", "-60"]
    assert f0.main([str(ev), "--data-dir", str(data), "--json", str(out)] + args) == 0
    printed = json.loads(capsys.readouterr().out)
    res = json.load(open(out))
    assert (res["n_scored"], res["n_empty"], res["n_without_target"]) == (5, 1, 1) and res["without_target"] == ["spk9_99"]
    assert printed["n_scored"] == 5 and "records" not in printed and printed["metric"] == "f0_dtw"
    assert all(printed[k] == res[k] for k in f0.SCORES)
    recs = {r["name"]: r for r in res["records"]}
    assert sorted(recs) == names
    # the same pairs in the same batches of 4 through the list function (checked against the oracle above)
    want = []
    for part in (slice(0, 4), slice(4, 6)):
        preds, pl = rescore.pad(gen[part], names[part], 80, "generated")
        targets, tl = rescore.pad(truth[part], names[part], 80, "target")
        want += f0.calculate_f0_dtw(preds, pl, targets, tl, n_iter=4, hp=hp, threshold=0.3, silence_db=-60.0)
    for n, l, w in zip(names, langs, want):
        r = recs[n]
        assert r["language"] == l
        if w is None:
            assert n == names[5] and not r["scored"] and r["ffe"] is None and r["steps"] is None
            continue
        assert r["scored"] and all(r[k] == w[k] for k in f0.COUNTS)
        assert all(r[k] == w[k] or (r[k] is None and np.isnan(w[k])) for k in f0.SCORES)
    for l in ("en-us", "de-de"):
        mine = [recs[n] for n, ll in zip(names, langs) if ll == l and recs[n]["scored"]]
        assert res["languages"][l]["n"] == len(mine)
        for k in f0.SCORES:
            v = [r[k] for r in mine if r[k] is not None]
            assert res["languages"][l][k] == (float(np.mean(v)) if v else None)
    v = [r["ffe"] for r in res["records"] if r["scored"]]
    assert res["ffe"] == float(np.mean(v))
    assert f0.main([str(ev), "--data-dir", str(data), "--radius", "exact"] + args) == 0
    assert json.loads(capsys.readouterr().out)["radius"] == "exact"
