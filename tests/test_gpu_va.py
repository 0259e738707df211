"""GPU tests of the variance adaptor (b2s_hip.variance, libb2s_va.so) against the NumPy restatement tests/va_ref.py.

The gate is equality throughout: integers EQUAL, fp32 compared as int32 bit patterns.  Every addition of the calls is specified
(include/b2s_va.h), so there is no tolerance to derive: anything but equality is a defect.  Every output is pre-filled with a
sentinel and has guard rows behind it, and so has the workspace; those must stay untouched.  The inputs never let +inf meet -inf,
so no NaN is made (the payload of a NaN is outside the contract)."""
import functools
import json

import numpy as np
import pytest
import torch

import va_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = np.float32(-7.5)                  # what an output holds before the call
GUARD = 3
BS, SS, DS, NBS = [1, 5], [1, 2, 65, 257], [4, 12, 68, 256, 768], [1, 2, 256]


def dev(a, dtype):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(DEV)     # a copy: the cases are read-only


def ptr(t):
    return None if t is None else t.data_ptr()


def same_bits(got, want):
    return np.array_equal(R.bits(got), R.bits(want))


def durations(rng, n, S, kind):
    """S durations of which the first n count: zeros at the start, the end and in runs, one position of 700 frames."""
    d = rng.integers(0, 6, size=S).astype(np.int32)
    d[rng.random(S) < 0.3] = 0
    if kind == "noframes":
        d[:] = 0
    elif n >= 1:
        d[0] = 0
        d[n - 1] = 0
        if n >= 8:
            d[3:6] = 0
        if kind == "long":
            d[n // 2] = 700                                                # more than any workgroup's worth of frames
        if n <= 2:
            d[n - 1] = 3 if kind != "long" else 700                        # otherwise S = 1, 2 would have no frame at all
    d[n:] = 9                                                              # behind the length: never looked at
    return d


@functools.lru_cache(maxsize=None)
def case(B, S, D, n_bins, seed=0):
    """Inputs of one batch and what the restatement makes of them (computed once, read-only)."""
    rng = np.random.default_rng(1000 * seed + 7 * B + 11 * S + 13 * D + n_bins)
    n = np.array([S, max(S // 2, 1), S, 1, max(S - 1, 1)][:B], np.int32)
    kinds = ["long", "plain", "noframes", "plain", "plain"][:B]
    dur = np.stack([durations(rng, int(n[b]), S, kinds[b]) for b in range(B)])
    off = R.offsets(dur, n)
    total = int(off[-1])
    c = {"B": B, "S": S, "D": D, "n_bins": n_bins, "n": n, "dur": dur, "off": off, "total": total,
         "x": rng.standard_normal((B, S, D)).astype(np.float32), "pt": rng.standard_normal((n_bins, D)).astype(np.float32),
         "et": rng.standard_normal((n_bins, D)).astype(np.float32), "pb": rng.integers(0, n_bins, size=(B, S)).astype(np.int32),
         "eb": rng.integers(0, n_bins, size=(B, S)).astype(np.int32), "dy": rng.standard_normal((total, D)).astype(np.float32)}
    c["pb"][:, 0], c["eb"][:, 0] = 0, n_bins - 1                           # the first and the last bin are used
    c["pb"][:, S - 1], c["eb"][:, S - 1] = n_bins - 1, 0
    c["x"][0, 0, 0] = -0.0
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def variant(c, **over):
    """A writable copy of a case with some arrays replaced."""
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    out.update(over)
    return out


def run_forward(c, pitch=True, energy=True, want_h=True, want_uof=True):
    """b2s_va_forward through the C ABI -> dict of host arrays (h, y, unit_of_frame, status); the guards are checked here."""
    from b2s_hip import variance
    l = variance.load()
    B, S, D, total = c["B"], c["S"], c["D"], c["total"]
    x, dur, n, off = dev(c["x"], np.float32), dev(c["dur"], np.int32), dev(c["n"], np.int32), dev(c["off"], np.int32)
    pb, pt = (dev(c["pb"], np.int32), dev(c["pt"], np.float32)) if pitch else (None, None)
    eb, et = (dev(c["eb"], np.int32), dev(c["et"], np.float32)) if energy else (None, None)
    h = torch.full((B * S + GUARD, D), float(SENT), dtype=torch.float32, device=DEV) if want_h else None
    y = torch.full((total + GUARD, D), float(SENT), dtype=torch.float32, device=DEV)
    uof = torch.full((total + GUARD,), -7, dtype=torch.int32, device=DEV) if want_uof else None
    st = torch.full((B + GUARD,), -7, dtype=torch.int32, device=DEV)
    variance.check(l.b2s_va_forward(ptr(x), ptr(pb), ptr(eb), ptr(pt), ptr(et), c["n_bins"], ptr(dur), ptr(n), ptr(off), total, B, S, D,
                                    ptr(h), ptr(y) if total else None, ptr(uof) if total else None, ptr(st), None))
    torch.cuda.synchronize()
    out = {"y": y.cpu().numpy(), "status": st.cpu().numpy()}
    assert np.all(out["y"][total:] == SENT) and np.all(out["status"][B:] == -7)
    out["y"], out["status"] = out["y"][:total], out["status"][:B]
    if want_h:
        hh = h.cpu().numpy()
        assert np.all(hh[B * S:] == SENT)
        out["h"] = hh[:B * S].reshape(B, S, D)
    if want_uof:
        u = uof.cpu().numpy()
        assert np.all(u[total:] == -7)
        out["unit_of_frame"] = u[:total]
    return out


def ref_forward(c, pitch=True, energy=True):
    return R.forward(c["x"], c["pb"] if pitch else None, c["eb"] if energy else None, c["pt"] if pitch else None,
                     c["et"] if energy else None, c["dur"], c["n"], c["off"], c["total"], sentinel=SENT)


def check_forward(got, want):
    assert np.array_equal(got["status"], want["status"])
    assert same_bits(got["y"], want["y"])
    if "h" in got:
        assert same_bits(got["h"], want["h"])
    if "unit_of_frame" in got:
        assert np.array_equal(got["unit_of_frame"], np.where(want["unit_of_frame"] < 0, -7, want["unit_of_frame"]))


def run_backward(c, pitch=True, energy=True, pitch_grad=True, energy_grad=True, ws_shift=4):
    """b2s_va_backward through the C ABI -> dict of host arrays.  The table gradients are pre-filled with garbage, dx and the
    workspace with sentinels; the workspace starts `ws_shift` bytes behind a 16-byte boundary."""
    from b2s_hip import variance
    l = variance.load()
    B, S, D, total, nb = c["B"], c["S"], c["D"], c["total"], c["n_bins"]
    dy = torch.cat([dev(c["dy"], np.float32).reshape(total, D), torch.full((GUARD, D), float("nan"), device=DEV)])
    dur, n, off = dev(c["dur"], np.int32), dev(c["n"], np.int32), dev(c["off"], np.int32)
    pb = dev(c["pb"], np.int32) if pitch else None
    eb = dev(c["eb"], np.int32) if energy else None
    dx = torch.full((B * S + GUARD, D), float(SENT), dtype=torch.float32, device=DEV)
    dpt = torch.full((nb + GUARD, D), 1e30, dtype=torch.float32, device=DEV) if pitch and pitch_grad else None
    det = torch.full((nb + GUARD, D), -1e30, dtype=torch.float32, device=DEV) if energy and energy_grad else None
    st = torch.full((B + GUARD,), -7, dtype=torch.int32, device=DEV)
    need = l.b2s_va_ws_bytes(B, S, D, nb)
    assert need > 0
    ws = torch.full((ws_shift + need + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 16 == 0
    variance.check(l.b2s_va_backward(ptr(dy), ptr(pb), ptr(eb), nb, ptr(dur), ptr(n), ptr(off), total, B, S, D, ptr(dx), ptr(dpt), ptr(det),
                                     ptr(st), ws.data_ptr() + ws_shift, need, None))
    torch.cuda.synchronize()
    w = ws.cpu().numpy()
    assert np.all(w[:ws_shift] == 0x5A) and np.all(w[ws_shift + need:] == 0x5A)
    out = {"dx": dx.cpu().numpy(), "status": st.cpu().numpy()}
    assert np.all(out["dx"][B * S:] == SENT) and np.all(out["status"][B:] == -7)
    out["dx"], out["status"] = out["dx"][:B * S].reshape(B, S, D), out["status"][:B]
    for name, t, fill in (("d_pitch_table", dpt, np.float32(1e30)), ("d_energy_table", det, np.float32(-1e30))):
        out[name] = None
        if t is not None:
            a = t.cpu().numpy()
            assert np.all(a[nb:] == fill)
            out[name] = a[:nb]
    return out


def ref_backward(c, pitch=True, energy=True):
    return R.backward(c["dy"], c["pb"] if pitch else None, c["eb"] if energy else None, c["n_bins"], c["dur"], c["n"], c["off"], c["total"],
                      D=c["D"])


def check_backward(got, want):
    assert np.array_equal(got["status"], want["status"])
    assert same_bits(got["dx"], want["dx"])
    for name in ("d_pitch_table", "d_energy_table"):
        if got[name] is not None:
            assert same_bits(got[name], want[name]), name


# ------------------------------------------------------------------------------------------------------ forward and backward

@pytest.mark.parametrize("n_bins", NBS)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("S", SS)
@pytest.mark.parametrize("B", BS)
def test_forward_equals_the_restatement(B, S, D, n_bins):
    c = case(B, S, D, n_bins)
    want = ref_forward(c)
    assert R.FAILED not in want["status"] and (B == 1 or want["status"][2] == R.OK and c["off"][3] == c["off"][2])   # 0 frames, n > 0
    check_forward(run_forward(c), want)


@pytest.mark.parametrize("n_bins", NBS)
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("S", SS)
@pytest.mark.parametrize("B", BS)
def test_backward_equals_the_restatement(B, S, D, n_bins):
    c = case(B, S, D, n_bins)
    check_backward(run_backward(c), ref_backward(c))


def test_all_four_waves_of_the_scan_at_the_largest_s():
    c = case(2, 1024, 4, 256)
    assert c["n"].tolist() == [1024, 512]
    check_forward(run_forward(c), ref_forward(c))
    check_backward(run_backward(c), ref_backward(c))


@pytest.mark.parametrize("pitch,energy", [(True, False), (False, True), (False, False)])
def test_a_table_that_is_null_is_not_added(pitch, energy):
    c = case(5, 65, 68, 256)
    got = run_forward(c, pitch, energy)
    check_forward(got, ref_forward(c, pitch, energy))
    if not pitch and not energy:
        assert R.bits(got["h"])[0, 0, 0] == np.int32(-2 ** 31)             # the -0.0 of x is kept: nothing was added to it
    check_backward(run_backward(c, pitch, energy), ref_backward(c, pitch, energy))
    # bins given, their gradient not asked for: dx and the other table are what they were
    got = run_backward(c, True, True, pitch_grad=pitch, energy_grad=energy)
    want = ref_backward(c)
    assert (got["d_pitch_table"] is None) == (not pitch) and (got["d_energy_table"] is None) == (not energy)
    check_backward(got, want)


def test_a_minus_zero_of_x_is_kept_through_the_frames():
    c = variant(case(1, 2, 4, 1))
    c["x"][:] = -0.0
    got = run_forward(c, False, False)
    assert c["total"] > 0 and np.all(R.bits(got["y"]) == np.int32(-2 ** 31)) and np.all(R.bits(got["h"]) == np.int32(-2 ** 31))
    c["pt"][:] = 0.0
    got = run_forward(c, True, False)
    assert np.all(R.bits(got["y"]) == 0)                                   # adding +0.0 is not adding nothing


def test_h_and_unit_of_frame_may_be_null():
    c = case(5, 65, 12, 2)
    want = ref_forward(c)
    for want_h, want_uof in ((False, True), (True, False), (False, False)):
        check_forward(run_forward(c, want_h=want_h, want_uof=want_uof), want)


def test_no_frame_in_the_whole_batch():
    c = variant(case(5, 65, 12, 2))
    c["dur"][:] = 0
    c["off"] = np.zeros(6, np.int32)
    c["total"] = 0
    c["dy"] = np.zeros((0, 12), np.float32)
    c["n"][3] = 0
    want = ref_forward(c)
    assert want["status"].tolist() == [R.OK, R.OK, R.OK, R.EMPTY, R.OK]
    got = run_forward(c)
    check_forward(got, want)
    assert not got["h"][3].any()
    gb = run_backward(c)
    check_backward(gb, ref_backward(c))
    assert not gb["dx"].any() and not gb["d_pitch_table"].any() and not gb["d_energy_table"].any()


def test_infinities_pass_through():
    c = variant(case(5, 65, 68, 2))
    c["x"][:, ::7, 0], c["x"][:, ::5, 1] = np.inf, -np.inf                 # the tables are finite: no NaN
    got = run_forward(c)
    check_forward(got, ref_forward(c))
    assert np.isinf(got["y"]).any() and not np.isnan(got["y"]).any()
    c["dy"][::3, 0], c["dy"][::4, 1] = np.inf, -np.inf                     # one sign per column
    gb = run_backward(c)
    check_backward(gb, ref_backward(c))
    assert np.isinf(gb["dx"]).any() and np.isinf(gb["d_pitch_table"]).any() and not np.isnan(gb["d_pitch_table"]).any()


@pytest.mark.parametrize("D", [4, 768])
def test_every_position_in_one_bin_and_each_bin_once(D):
    """The longest chains (S = 257 rows into one partial sum, then B = 5 partial sums into one table row), and none at all."""
    c = variant(case(5, 257, D, 256))
    c["n"][:] = 257
    c["dur"][c["dur"] == 9] = 1
    c["off"] = R.offsets(c["dur"], c["n"])
    c["total"] = int(c["off"][-1])
    c["dy"] = np.random.default_rng(3).standard_normal((c["total"], D)).astype(np.float32)
    c["pb"][:] = 200
    c["eb"][:] = np.arange(257)[None, :] % 256                             # 255 bins once per utterance, bin 0 twice
    got = run_backward(c)
    check_backward(got, ref_backward(c))
    assert not got["d_pitch_table"][:200].any() and not got["d_pitch_table"][201:].any() and got["d_pitch_table"][200].all()
    check_forward(run_forward(c), ref_forward(c))


def test_alone_or_in_the_batch_and_twice():
    c = case(5, 65, 68, 256)
    full = run_backward(c)
    again = run_backward(c, ws_shift=12)
    for k in ("dx", "d_pitch_table", "d_energy_table"):
        assert same_bits(full[k], again[k])                                # the same bits from run to run
    fy = run_forward(c)
    for b in (0, 4):
        lo, hi = int(c["off"][b]), int(c["off"][b + 1])
        one = variant(c, B=1, n=c["n"][b:b + 1], dur=c["dur"][b:b + 1], x=c["x"][b:b + 1], pb=c["pb"][b:b + 1], eb=c["eb"][b:b + 1],
                      off=np.array([0, hi - lo], np.int32), total=hi - lo, dy=c["dy"][lo:hi])
        alone = run_backward(one)
        assert same_bits(alone["dx"][0], full["dx"][b])
        assert same_bits(run_forward(one)["y"], fy["y"][lo:hi])
        # the only OK utterance of the batch: the others get a length outside 0..S
        only = variant(c)
        only["n"][:] = -1
        only["n"][b] = c["n"][b]
        got = run_backward(only)
        assert got["status"].tolist() == [R.OK if i == b else R.FAILED for i in range(5)]
        assert same_bits(got["d_pitch_table"], alone["d_pitch_table"]) and same_bits(got["d_energy_table"], alone["d_energy_table"])
        assert same_bits(got["dx"][b], alone["dx"][0]) and not np.delete(got["dx"], b, axis=0).any()


# -------------------------------------------------------------------------------------------------------------------- statuses

def three(D=8, S=9, n_bins=4, seed=1):
    """Three utterances of a few frames each; the middle one is what the status tests break."""
    rng = np.random.default_rng(seed)
    n = np.array([S, S - 2, S - 1], np.int32)
    dur = rng.integers(0, 4, size=(3, S)).astype(np.int32)
    dur[:, 1] = 2
    off = R.offsets(dur, n)
    total = int(off[-1])
    return {"B": 3, "S": S, "D": D, "n_bins": n_bins, "n": n, "dur": dur, "off": off, "total": total,
            "x": rng.standard_normal((3, S, D)).astype(np.float32), "pt": rng.standard_normal((n_bins, D)).astype(np.float32),
            "et": rng.standard_normal((n_bins, D)).astype(np.float32), "pb": rng.integers(0, n_bins, size=(3, S)).astype(np.int32),
            "eb": rng.integers(0, n_bins, size=(3, S)).astype(np.int32), "dy": rng.standard_normal((total, D)).astype(np.float32)}


def without(c, b):
    """The batch without utterance b, its frames packed anew."""
    keep = [i for i in range(c["B"]) if i != b]
    rows = np.concatenate([np.arange(c["off"][i], c["off"][i + 1]) for i in keep]).astype(np.int64)
    fr = [int(c["off"][i + 1] - c["off"][i]) for i in keep]
    return variant(c, B=len(keep), n=c["n"][keep], dur=c["dur"][keep], x=c["x"][keep], pb=c["pb"][keep], eb=c["eb"][keep],
                   off=np.concatenate([[0], np.cumsum(fr)]).astype(np.int32), total=int(sum(fr)), dy=c["dy"][rows])


def break_n_negative(c):
    c["n"][1] = -1


def break_n_past_s(c):
    c["n"][1] = c["S"] + 1


def break_duration(c):
    c["dur"][1, 2] = -1                                                    # the offsets still claim the frames of before


def break_pitch_bin_high(c):
    c["pb"][1, 3] = c["n_bins"]


def break_energy_bin_negative(c):
    c["eb"][1, 0] = -1


def break_sum(c):
    c["dur"][1, 4] += 1                                                    # one frame more than the offsets give it


def break_offsets_decrease(c):
    f = [int(c["off"][i + 1] - c["off"][i]) for i in range(3)]
    # utterance 2 sits in front, two rows that belong to nobody, then utterance 0: utterance 1 runs from behind 0 back to row 0
    c["off"] = np.array([f[2] + 2, f[2] + 2 + f[0], 0, f[2]], np.int32)
    c["total"] = f[2] + 2 + f[0]
    c["dy"] = np.random.default_rng(9).standard_normal((c["total"], c["D"])).astype(np.float32)


BREAKS = [break_n_negative, break_n_past_s, break_duration, break_pitch_bin_high, break_energy_bin_negative, break_sum,
          break_offsets_decrease]


@pytest.mark.parametrize("how", BREAKS, ids=lambda f: f.__name__)
def test_one_failed_utterance_between_two_ok_ones(how):
    c = three()
    how(c)
    want = ref_forward(c)
    assert want["status"].tolist() == [R.OK, R.FAILED, R.OK]
    got = run_forward(c)
    check_forward(got, want)
    assert np.all(got["h"][1] == SENT)                                     # nothing but its status is written
    lo, hi = int(c["off"][1]), int(c["off"][2])
    if hi > lo:
        assert np.all(got["y"][lo:hi] == SENT) and np.all(got["unit_of_frame"][lo:hi] == -7)
    for b in (0, 2):
        assert not np.any(got["y"][c["off"][b]:c["off"][b + 1]] == SENT) and c["off"][b + 1] > c["off"][b]
    gb = run_backward(c)
    check_backward(gb, ref_backward(c))
    assert not gb["dx"][1].any() and gb["dx"][0].any() and gb["dx"][2].any()
    rest = ref_backward(without(c, 1))                                     # the restatement run without it
    assert rest["status"].tolist() == [R.OK, R.OK]
    assert same_bits(gb["dx"][[0, 2]], rest["dx"])
    assert same_bits(gb["d_pitch_table"], rest["d_pitch_table"]) and same_bits(gb["d_energy_table"], rest["d_energy_table"])


def test_offsets_that_leave_the_range_and_an_empty_utterance():
    c = three()
    c["off"] = c["off"].copy()
    c["off"][0] = -1                                                       # utterance 0 starts in front of the array
    want = ref_forward(c)
    assert want["status"].tolist() == [R.FAILED, R.OK, R.OK]
    check_forward(run_forward(c), want)
    check_backward(run_backward(c), ref_backward(c))
    c = three()
    c["total"] -= 1                                                        # utterance 2 ends behind it
    c["dy"] = c["dy"][:-1]
    want = ref_forward(c)
    assert want["status"].tolist() == [R.OK, R.OK, R.FAILED]
    check_forward(run_forward(c), want)
    check_backward(run_backward(c), ref_backward(c))
    c = three()
    c["n"][1] = 0                                                          # EMPTY, but the offsets give it frames: FAILED
    assert ref_forward(c)["status"].tolist() == [R.OK, R.FAILED, R.OK]
    check_forward(run_forward(c), ref_forward(c))
    c = without(three(), 1)
    c.update(B=3, n=np.array([c["n"][0], 0, c["n"][1]], np.int32), dur=c["dur"][[0, 0, 1]], x=c["x"][[0, 0, 1]], pb=c["pb"][[0, 0, 1]],
             eb=c["eb"][[0, 0, 1]], off=c["off"][[0, 1, 1, 2]])
    want = ref_forward(c)
    assert want["status"].tolist() == [R.OK, R.EMPTY, R.OK]
    got = run_forward(c)
    check_forward(got, want)
    assert not got["h"][1].any()
    gb = run_backward(c)
    check_backward(gb, ref_backward(c))
    assert not gb["dx"][1].any()


def test_more_frames_than_an_utterance_may_have():
    S, D = 2, 4
    big = R.MAX_FRAMES
    for d0, ok in ((big - 1, True), (big, False)):                         # the sum is MAX_FRAMES, and one more
        dur = np.array([[2, 1], [d0, 1]], np.int32)
        n = np.array([2, 2], np.int32)
        off = R.offsets(dur, n)
        total = int(off[-1])
        x = torch.randn(2, S, D, device=DEV)
        y = torch.full((total + GUARD, D), float(SENT), device=DEV)
        st = torch.full((2,), -7, dtype=torch.int32, device=DEV)
        from b2s_hip import variance
        l = variance.load()
        dd, nn, oo = dev(dur, np.int32), dev(n, np.int32), dev(off, np.int32)
        variance.check(l.b2s_va_forward(ptr(x), None, None, None, None, 1, ptr(dd), ptr(nn), ptr(oo), total, 2, S, D, None, ptr(y), None,
                                        ptr(st), None))
        torch.cuda.synchronize()
        assert st.cpu().tolist() == [R.OK, R.OK if ok else R.FAILED]
        assert R.statuses(None, None, 1, dur, n, off, total).tolist() == st.cpu().tolist()
        assert torch.equal(y[:2], x[0, :1].expand(2, D)) and torch.equal(y[2], x[0, 1]) and bool((y[total:] == float(SENT)).all())
        if ok:
            assert torch.equal(y[3:3 + d0], x[1, :1].expand(d0, D)) and torch.equal(y[3 + d0], x[1, 1])
        else:
            assert bool((y[3:] == float(SENT)).all())
        fr, fs = variance.frame_counts(dd, nn)
        assert fr.cpu().tolist() == [3, d0 + 1 if ok else 0] and fs.cpu().tolist() == [R.OK, R.OK if ok else R.FAILED]


# --------------------------------------------------------------------------------------------------------- quantise and frames

@pytest.mark.parametrize("n_bins", [1, 2, 16, 256])
def test_quantise_equals_the_restatement(n_bins):
    from b2s_hip import variance
    rng = np.random.default_rng(n_bins)
    bd = np.sort(rng.normal(size=n_bins - 1))
    v = rng.normal(size=(6, 300))
    k = min(n_bins - 1, 300)
    v[0, :k] = bd[:k]                                                      # exactly on a boundary
    v[1, 0], v[1, 1] = -np.inf, np.inf
    v[2, 150] = np.nan                                                     # among the first 300: FAILED
    v[3, 299] = np.nan                                                     # behind the length: not looked at
    n = [300, 300, 300, 299, 0, 301]
    bins, st = variance.quantise_batch(v, n, bd)
    wb, ws = R.quantise(v, n, bd)
    assert bins.dtype == torch.int32 and np.array_equal(bins.cpu().numpy(), wb) and np.array_equal(st.cpu().numpy(), ws)
    assert ws.tolist() == [R.OK, R.OK, R.FAILED, R.OK, R.EMPTY, R.FAILED]
    want = torch.bucketize(torch.from_numpy(v[:2]), torch.from_numpy(bd), right=False).numpy()
    assert np.array_equal(bins.cpu().numpy()[:2], want)
    if n_bins > 2:
        for bad in (bd[::-1].copy(), np.where(np.arange(n_bins - 1) == 1, bd[0], bd), np.where(np.arange(n_bins - 1) == n_bins - 2, np.inf, bd),
                    np.where(np.arange(n_bins - 1) == 0, np.nan, bd)):
            bins, st = variance.quantise_batch(v, n, bad)                  # not ascending, a tie, an infinity, a NaN: everyone FAILED
            assert st.cpu().tolist() == [R.FAILED] * 6 and not bins.cpu().numpy().any()
            assert R.quantise(v, n, bad)[1].tolist() == [R.FAILED] * 6


def test_frame_counts_equal_the_restatement():
    from b2s_hip import variance
    rng = np.random.default_rng(4)
    d = rng.integers(0, 9, size=(7, 1024)).astype(np.int32)
    d[2, 700] = -1
    d[3, :] = 1024                                                         # exactly MAX_FRAMES
    d[4, :] = 1024
    d[4, 5] = 1025                                                         # one more
    d[5, 3] = 2 ** 31 - 1
    n = [1024, 1, 701, 1024, 1024, 10, 0]
    fr, st = variance.frame_counts(d, n)
    wf, ws = R.frames(d, n)
    assert np.array_equal(fr.cpu().numpy(), wf) and np.array_equal(st.cpu().numpy(), ws)
    assert ws.tolist() == [R.OK, R.OK, R.FAILED, R.OK, R.FAILED, R.FAILED, R.EMPTY] and wf[3] == R.MAX_FRAMES


# ----------------------------------------------------------------------------------------------------------- the Python surface

def test_expand_under_autograd_equals_the_restatement():
    from b2s_hip import variance
    c = variant(case(5, 65, 68, 256))
    x = dev(c["x"], np.float32).requires_grad_(True)
    pt, et = dev(c["pt"], np.float32).requires_grad_(True), dev(c["et"], np.float32).requires_grad_(True)
    out = variance.expand(x, c["dur"], c["n"], (c["pb"], pt), (c["eb"], et))
    want = ref_forward(c)
    assert out["frame_offsets"].tolist() == c["off"].tolist() and out["frame_lengths"] == np.diff(c["off"]).tolist()
    assert same_bits(out["frames"].detach().cpu().numpy(), want["y"]) and out["status"].cpu().tolist() == want["status"].tolist()
    assert np.array_equal(out["unit_of_frame"].cpu().numpy(), want["unit_of_frame"])
    dy = dev(c["dy"], np.float32)
    (out["frames"] * dy).sum().backward()
    wb = ref_backward(c)
    assert same_bits(x.grad.cpu().numpy(), wb["dx"])
    assert same_bits(pt.grad.cpu().numpy(), wb["d_pitch_table"]) and same_bits(et.grad.cpu().numpy(), wb["d_energy_table"])
    # frame_lengths from the host: the same result; wrong ones: refused by name
    known = variance.expand(x, c["dur"], c["n"], (c["pb"], pt), (c["eb"], et), frame_lengths=np.diff(c["off"]).tolist())
    assert torch.equal(known["frames"], out["frames"])
    wrong = np.diff(c["off"]).tolist()
    wrong[1] += 1
    with pytest.raises(variance.B2SError, match=r"failed for utterances \[1\]"):
        variance.expand(x, c["dur"], c["n"], (c["pb"], pt), (c["eb"], et), frame_lengths=wrong)
    quiet = variance.expand(x, c["dur"], c["n"], (c["pb"], pt), (c["eb"], et), frame_lengths=wrong, check_status=False)
    assert quiet["status"].cpu().tolist() == [R.OK, R.FAILED, R.OK, R.OK, R.OK]
    # one table only, and none
    x2 = dev(c["x"], np.float32).requires_grad_(True)
    only = variance.expand(x2, c["dur"], c["n"], energy=(c["eb"], et.detach()))
    assert same_bits(only["frames"].detach().cpu().numpy(), ref_forward(c, False, True)["y"])
    (only["frames"] * dy).sum().backward()                                 # the table asks for no gradient
    assert same_bits(x2.grad.cpu().numpy(), wb["dx"])
    none = variance.expand(x2.detach(), c["dur"], c["n"])
    assert same_bits(none["frames"].cpu().numpy(), ref_forward(c, False, False)["y"])


def integer_module(n_bins=8, D=12, B=3, S=9, seed=5):
    from b2s_hip import variance
    rng = np.random.default_rng(seed)
    pbd, ebd = np.arange(1, n_bins) * 50.0, np.arange(1, n_bins) * 0.5
    va = variance.VarianceAdaptor(n_bins, D, pbd, ebd).to(DEV)
    with torch.no_grad():
        va.pitch_embedding.weight.copy_(dev(rng.integers(-8, 9, size=(n_bins, D)), np.float32))
        va.energy_embedding.weight.copy_(dev(rng.integers(-8, 9, size=(n_bins, D)), np.float32))
    pitch = rng.uniform(0, 50.0 * n_bins, size=(B, S))
    pitch[0, :3] = [50.0, 100.0, 0.0]                                      # on a boundary: the bin below
    energy = rng.uniform(0, 0.5 * n_bins, size=(B, S))
    dur = rng.integers(0, 5, size=(B, S)).astype(np.int32)
    n = np.array([S, S - 4, 1], np.int32)
    x = rng.integers(-8, 9, size=(B, S, D)).astype(np.float32)
    return va, pbd, ebd, pitch, energy, dur, n, x


def test_the_module_under_autograd_and_a_second_backward_doubles_the_gradients():
    va, pbd, ebd, pitch, energy, dur, n, x = integer_module()
    assert va.pitch_boundaries.dtype == torch.float64 and va.pitch_boundaries.is_cuda
    xt = dev(x, np.float32).requires_grad_(True)
    out = va(xt, pitch, energy, dur, n)
    pb, _ = R.quantise(pitch, n, pbd)
    eb, _ = R.quantise(energy, n, ebd)
    assert np.array_equal(out["pitch_bins"].cpu().numpy(), pb) and np.array_equal(out["energy_bins"].cpu().numpy(), eb)
    assert pb[0, :3].tolist() == [0, 1, 0]
    off = R.offsets(dur, n)
    total = int(off[-1])
    pt, et = va.pitch_embedding.weight.detach().cpu().numpy(), va.energy_embedding.weight.detach().cpu().numpy()
    want = R.forward(x, pb, eb, pt, et, dur, n, off, total)
    assert same_bits(out["frames"].detach().cpu().numpy(), want["y"]) and out["frame_offsets"].tolist() == off.tolist()
    dy = np.random.default_rng(6).integers(-8, 9, size=(total, x.shape[2])).astype(np.float32)
    loss = (out["frames"] * dev(dy, np.float32)).sum()
    loss.backward(retain_graph=True)
    wb = R.backward(dy, pb, eb, va.n_bins, dur, n, off, total)
    grads = (xt.grad, va.pitch_embedding.weight.grad, va.energy_embedding.weight.grad)
    for g, w in zip(grads, (wb["dx"], wb["d_pitch_table"], wb["d_energy_table"])):
        assert same_bits(g.cpu().numpy(), w)
    loss.backward()                                                        # accumulates: integers, so exactly twice
    for g, w in zip((xt.grad, va.pitch_embedding.weight.grad, va.energy_embedding.weight.grad),
                    (wb["dx"], wb["d_pitch_table"], wb["d_energy_table"])):
        assert same_bits(g.cpu().numpy(), (2 * w).astype(np.float32))
    # a NaN target fails its utterance by name
    pitch[1, 0] = np.nan
    from b2s_hip import B2SError
    with pytest.raises(B2SError, match=r"failed for utterances \[1\]"):
        va(xt, pitch, energy, dur, n)


def test_padded_and_its_backward():
    from b2s_hip import variance
    c = variant(case(5, 65, 68, 256))
    frames = dev(c["dy"], np.float32).requires_grad_(True)
    T = int(np.diff(c["off"]).max()) + 3
    out = variance.padded(frames, c["off"], T)
    assert out.shape == (5, T, 68)
    host = out.detach().cpu().numpy()
    for b in range(5):
        lo, hi = int(c["off"][b]), int(c["off"][b + 1])
        assert same_bits(host[b, :hi - lo], c["dy"][lo:hi]) and np.all(R.bits(host[b, hi - lo:]) == 0)
    g = torch.randn(5, T, 68, device=DEV)
    (out * g).sum().backward()
    gh = g.cpu().numpy()
    want = np.concatenate([gh[b, :int(c["off"][b + 1] - c["off"][b])] for b in range(5)])
    assert same_bits(frames.grad.cpu().numpy(), want)
    # the C call: more frames than T is FAILED and leaves the block alone; guards stay
    l = variance.load()
    off = dev([0, 3, 3, 9], np.int32)
    fr = torch.randn(9, 4, device=DEV)
    block = torch.full((3 * 4 + GUARD, 4), float(SENT), device=DEV)
    st = torch.full((3 + GUARD,), -7, dtype=torch.int32, device=DEV)
    variance.check(l.b2s_va_pad(ptr(fr), ptr(off), 9, 3, 4, 4, ptr(block), 0, ptr(st), None))
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [R.OK, R.EMPTY, R.FAILED] + [-7] * GUARD
    assert torch.equal(block[:3], fr[:3]) and not block[3:8].any() and bool((block[8:] == float(SENT)).all())


def test_through_the_file_formats(tmp_path):
    """Three utterances in the layout prosody.extract writes, and its stats.json: boundaries, module, forward."""
    from b2s_hip import prosody, variance
    rng = np.random.default_rng(8)
    units, rows = [7, 12, 4], []
    for i, nu in enumerate(units):
        fr = rng.integers(0, 9, size=nu).astype(np.int32)
        pitch = np.where(fr > 0, rng.uniform(80, 300, size=nu), 0.0)
        energy = np.where(fr > 0, rng.uniform(1e3, 1e7, size=nu), 0.0)
        np.savez(str(tmp_path / ("utt%d.npz" % i)), duration=fr, pitch=pitch, pitch_voiced=pitch, voiced_frames=fr, energy=energy)
        rows.append(("en", fr, pitch, energy))
    with open(str(tmp_path / "stats.json"), "w") as f:
        json.dump(dict(prosody.unit_stats(rows, 800), units="bytes", utterances=3), f)
    n_bins, D, S = 16, 12, max(units)
    va = variance.VarianceAdaptor(n_bins, D, variance.boundaries_from_stats(str(tmp_path / "stats.json"), "pitch", n_bins),
                                  variance.boundaries_from_stats(str(tmp_path / "stats.json"), "energy", n_bins)).to(DEV)
    dur, pitch, energy = np.zeros((3, S), np.int32), np.zeros((3, S)), np.zeros((3, S))
    for i, nu in enumerate(units):
        z = np.load(str(tmp_path / ("utt%d.npz" % i)))
        dur[i, :nu], pitch[i, :nu], energy[i, :nu] = z["duration"], z["pitch"], z["energy"]
    x = torch.randn(3, S, D, device=DEV)
    out = va(x, pitch, energy, dur, units)
    assert out["status"].cpu().tolist() == [R.OK] * 3
    assert out["frame_lengths"] == [int(r[1].sum()) for r in rows] and out["frames"].shape == (sum(out["frame_lengths"]), D)
    pb = out["pitch_bins"].cpu().numpy()
    assert pb.min() == 0 and pb.max() == n_bins - 1                        # the overall minimum and maximum sit in the end bins
    want = R.forward(x.cpu().numpy(), pb, out["energy_bins"].cpu().numpy(), va.pitch_embedding.weight.detach().cpu().numpy(),
                     va.energy_embedding.weight.detach().cpu().numpy(), dur, units, out["frame_offsets"], int(out["frame_offsets"][-1]))
    assert same_bits(out["frames"].detach().cpu().numpy(), want["y"])
    assert np.array_equal(out["unit_of_frame"].cpu().numpy(), want["unit_of_frame"])
