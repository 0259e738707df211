"""GPU tests of the variance predictor (b2s_hip.predictor, libb2s_vp.so) against the NumPy restatement tests/vp_ref.py.

The gate is equality throughout: fp32 compared as int32 bit patterns.  Every operation of the calls is specified (include/b2s_vp.h),
so there is no tolerance to derive: anything but equality is a defect.  Every output is pre-filled with a sentinel and has guard rows
behind it, and so have the tape and the workspace; those must stay untouched."""
import functools

import numpy as np
import pytest
import torch

import vp_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = np.float32(-7.5)                  # what an output holds before the call
GUARD = 3                                # rows behind every output
GUARD_BYTES = 512                        # behind the tape and the workspace
EPS = 1e-5
NAMES = ("W1", "b1", "g1", "be1", "W2", "b2", "g2", "be2", "wl", "bl")
GRADS = tuple("d" + k for k in NAMES)


def dev(a, dtype):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(DEV)     # a copy: the cases are read-only


def ptr(t):
    return None if t is None else t.data_ptr()


def same_bits(got, want):
    return np.array_equal(R.bits(got), R.bits(want))


def lengths_of(B, S):
    return np.array([S, max(S // 2, 1), 1][:B], np.int32)


def make_inputs(B, S, D, F, n, seed=0):
    rng = np.random.default_rng(1000 * seed + 7 * B + 11 * S + 13 * D + F)
    c = {"B": B, "S": S, "D": D, "F": F, "n": np.asarray(n, np.int32),
         "x": rng.standard_normal((B, S, D)).astype(np.float32), "d_pred": rng.standard_normal((B, S)).astype(np.float32),
         "W1": (rng.standard_normal((F, D, 3)) / np.sqrt(3 * D)).astype(np.float32), "b1": (0.3 * rng.standard_normal(F)).astype(np.float32),
         "g1": (1 + 0.2 * rng.standard_normal(F)).astype(np.float32), "be1": (0.2 * rng.standard_normal(F)).astype(np.float32),
         "W2": (rng.standard_normal((F, F, 3)) / np.sqrt(3 * F)).astype(np.float32), "b2": (0.3 * rng.standard_normal(F)).astype(np.float32),
         "g2": (1 + 0.2 * rng.standard_normal(F)).astype(np.float32), "be2": (0.2 * rng.standard_normal(F)).astype(np.float32),
         "wl": (rng.standard_normal(F) / np.sqrt(F)).astype(np.float32), "bl": (0.3 * rng.standard_normal(1)).astype(np.float32)}
    c["x"][0, 0, 0] = -0.0
    c["b1"][0] = -0.0
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def case(B, S, D, F):
    return make_inputs(B, S, D, F, lengths_of(B, S))


@functools.lru_cache(maxsize=None)
def reference(B, S, D, F, p, seed=11):
    """What the restatement makes of case(B, S, D, F): (forward, backward), computed once."""
    return ref_both(case(B, S, D, F), p, seed)


def ref_both(c, p, seed):
    fwd = R.forward(c["x"], c["n"], c, EPS, p=p, seed=seed, sentinel=SENT)
    return fwd, R.backward(c["x"], c["n"], c, fwd, c["d_pred"])


def guarded_bytes(nbytes, shift=0):
    """A byte buffer of `nbytes` behind `shift` bytes, full of 0xA5, with guard bytes on both sides."""
    whole = torch.full((GUARD_BYTES + shift + nbytes + GUARD_BYTES,), 0xA5, dtype=torch.uint8, device=DEV)
    return whole, whole[GUARD_BYTES + shift:GUARD_BYTES + shift + nbytes]


def guards_untouched(whole, nbytes, shift=0):
    h = whole.cpu().numpy()
    return bool(np.all(h[:GUARD_BYTES + shift] == 0xA5) and np.all(h[GUARD_BYTES + shift + nbytes:] == 0xA5))


def run_forward(c, p=0.0, seed=11, want_tape=True, ws_shift=4):
    """b2s_vp_forward through the C ABI -> dict (pred, status as host arrays; the device tape and parameters for backward)."""
    from b2s_hip import predictor
    l = predictor.load()
    B, S, D, F = c["B"], c["S"], c["D"], c["F"]
    x, n = dev(c["x"], np.float32), dev(c["n"], np.int32)
    params = [dev(c[k], np.float32) for k in NAMES]
    pred = torch.full((B * S + GUARD,), float(SENT), dtype=torch.float32, device=DEV)
    st = torch.full((B + GUARD,), -7, dtype=torch.int32, device=DEV)
    ws_n, tape_n = l.b2s_vp_ws_bytes(B, S, D, F), l.b2s_vp_tape_bytes(B, S, F)
    assert ws_n == R.ws_bytes(B, S, D, F) and tape_n == R.tape_bytes(B, S, F)
    ws_whole, ws = guarded_bytes(ws_n, ws_shift)
    tape_whole, tape = guarded_bytes(tape_n) if want_tape else (None, None)
    predictor.check(l.b2s_vp_forward(ptr(x), ptr(n), *[ptr(t) for t in params], EPS, p, seed, B, S, D, F, ptr(pred), ptr(st), ptr(tape),
                                     ptr(ws), ws_n, None))
    torch.cuda.synchronize()
    out = {"pred": pred.cpu().numpy(), "status": st.cpu().numpy(), "tape": tape, "x": x, "n": n, "params": params}
    assert np.all(out["pred"][B * S:] == SENT) and np.all(out["status"][B:] == -7)
    assert guards_untouched(ws_whole, ws_n, ws_shift)
    if want_tape:
        assert guards_untouched(tape_whole, tape_n)
    out["pred"], out["status"] = out["pred"][:B * S].reshape(B, S), out["status"][:B]
    return out


def run_backward(c, fwd, p=0.0, seed=11, want_dx=True, want_grads=True, ws_shift=4):
    """b2s_vp_backward through the C ABI on the tape of `fwd` -> dict of host arrays; outputs start as sentinels or garbage."""
    from b2s_hip import predictor
    l = predictor.load()
    B, S, D, F = c["B"], c["S"], c["D"], c["F"]
    d_pred = dev(c["d_pred"], np.float32)
    dx = torch.full((B * S + GUARD, D), float(SENT), dtype=torch.float32, device=DEV) if want_dx else None
    shapes = [c[k].shape for k in NAMES]
    grads = [torch.full((int(np.prod(s)) + GUARD,), 1e30, dtype=torch.float32, device=DEV) for s in shapes] if want_grads else [None] * 10
    ws_n = l.b2s_vp_ws_bytes(B, S, D, F)
    ws_whole, ws = guarded_bytes(ws_n, ws_shift)
    tape_before = fwd["tape"].clone()
    predictor.check(l.b2s_vp_backward(ptr(fwd["x"]), ptr(fwd["n"]), *[ptr(t) for t in fwd["params"]], ptr(fwd["tape"]), ptr(d_pred), p, seed,
                                      B, S, D, F, ptr(dx), *[ptr(g) for g in grads], ptr(ws), ws_n, None))
    torch.cuda.synchronize()
    assert guards_untouched(ws_whole, ws_n, ws_shift)
    assert torch.equal(tape_before, fwd["tape"])                           # backward only reads the tape
    out = {}
    if want_dx:
        h = dx.cpu().numpy()
        assert np.all(h[B * S:] == SENT)
        out["dx"] = h[:B * S].reshape(B, S, D)
    if want_grads:
        for name, g, s in zip(GRADS, grads, shapes):
            h = g.cpu().numpy()
            assert np.all(h[int(np.prod(s)):] == np.float32(1e30)), name
            out[name] = h[:int(np.prod(s))].reshape(s)
    return out


def check_backward(got, want):
    for k, v in got.items():
        assert same_bits(v, want[k]), "%s: %d of %d elements differ" % (k, np.count_nonzero(R.bits(v) != R.bits(want[k])), v.size)


def check_forward(got, want):
    assert np.array_equal(got["status"], want["status"])
    assert same_bits(got["pred"], want["pred"]), "%d of %d pred differ" % (
        np.count_nonzero(R.bits(got["pred"]) != R.bits(want["pred"])), got["pred"].size)


# ------------------------------------------------------------------------------------------------------ forward and backward

@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("F", [64, 256])
@pytest.mark.parametrize("D", [4, 36, 68])
@pytest.mark.parametrize("S", [1, 2, 3, 33, 65])
@pytest.mark.parametrize("B", [1, 3])
def test_forward_and_backward_are_the_restatement(B, S, D, F, p):
    c = case(B, S, D, F)
    want_f, want_b = reference(B, S, D, F, p)
    fwd = run_forward(c, p)
    check_forward(fwd, want_f)
    check_backward(run_backward(c, fwd, p), want_b)


def test_a_k_walk_over_several_lds_stages():
    c = case(3, 33, 260, 128)
    want_f, want_b = reference(3, 33, 260, 128, 0.5)
    fwd = run_forward(c, 0.5)
    check_forward(fwd, want_f)
    check_backward(run_backward(c, fwd, 0.5), want_b)


@pytest.mark.parametrize("B,F", [(3, 128), (1, 512)])
def test_the_other_filter_sizes(B, F):
    c = case(B, 33, 36, F)
    want_f, want_b = reference(B, 33, 36, F, 0.5)
    fwd = run_forward(c, 0.5)
    check_forward(fwd, want_f)
    check_backward(run_backward(c, fwd, 0.5), want_b)


@pytest.mark.parametrize("B,S,D,F,p", [(3, 65, 68, 64, 0.5), (1, 3, 4, 256, 0.0), (3, 33, 36, 256, 0.5)])
def test_dx_null_and_gradients_null(B, S, D, F, p):
    c = case(B, S, D, F)
    _, want_b = reference(B, S, D, F, p)
    fwd = run_forward(c, p)
    got = run_backward(c, fwd, p, want_dx=False)
    assert "dx" not in got and len(got) == 10
    check_backward(got, want_b)
    got = run_backward(c, fwd, p, want_grads=False)
    assert list(got) == ["dx"]
    check_backward(got, want_b)


@pytest.mark.parametrize("B,S,D,F,p", [(3, 65, 68, 64, 0.5), (1, 1, 4, 64, 0.0), (3, 33, 36, 256, 0.5)])
def test_inference_without_a_tape(B, S, D, F, p):
    check_forward(run_forward(case(B, S, D, F), p, want_tape=False), reference(B, S, D, F, p)[0])


def test_an_utterance_alone_has_the_rows_it_has_in_the_batch():
    B, S, D, F = 3, 65, 68, 64
    c = case(B, S, D, F)
    for b, p in ((0, 0.5), (1, 0.0), (2, 0.0)):                            # the dropout index counts from the batch's first row
        fwd = run_forward(c, p)
        dx = run_backward(c, fwd, p, want_grads=False)["dx"]
        alone = dict(c, B=1, n=c["n"][b:b + 1], x=c["x"][b:b + 1], d_pred=c["d_pred"][b:b + 1])
        fwd1 = run_forward(alone, p)
        dx1 = run_backward(alone, fwd1, p, want_grads=False)["dx"]
        assert same_bits(fwd1["pred"][0], fwd["pred"][b]) and same_bits(dx1[0], dx[b])


def test_two_runs_give_the_same_bits():
    c = case(3, 65, 68, 256)
    runs = []
    for _ in range(2):
        fwd = run_forward(c, 0.5)
        runs.append(dict(run_backward(c, fwd, 0.5), pred=fwd["pred"]))
    for k in runs[0]:
        assert same_bits(runs[0][k], runs[1][k]), k


@pytest.mark.parametrize("p,seed,site,B,S,F", [(0.5, 11, 1, 3, 65, 64), (0.5, 11, 2, 3, 65, 64), (0.1, (1 << 40) + 5, 1, 2, 33, 256),
                                               (0.0, 3, 2, 1, 2, 128), (0.999, 2 ** 64 - 1, 2, 1, 1024, 512)])
def test_the_device_mask_is_the_restatement(p, seed, site, B, S, F):
    from b2s_hip import predictor
    got = predictor.dropout_mask(p, seed, site, B, S, F).cpu().numpy()
    want = R.mask(p, seed, site, B, S, F)
    assert got.dtype == np.uint8 and np.array_equal(got, want.astype(np.uint8))
    if p == 0.0:
        assert got.all()


# ----------------------------------------------------------------------------------------------------------- EMPTY and FAILED

@pytest.mark.parametrize("p", [0.0, 0.5])
def test_empty_and_failed_utterances_among_ok_ones(p):
    B, S, D, F = 5, 33, 36, 64
    c = make_inputs(B, S, D, F, [S, -1, 0, S + 1, S // 2], seed=3)
    want_f, want_b = ref_both(c, p, 11)
    assert want_f["status"].tolist() == [R.OK, R.FAILED, R.EMPTY, R.FAILED, R.OK]
    fwd = run_forward(c, p)
    check_forward(fwd, want_f)
    assert np.all(fwd["pred"][[1, 3]] == SENT) and not fwd["pred"][2].any()          # nothing but the status; zeros
    got = run_backward(c, fwd, p)
    check_backward(got, want_b)
    assert not got["dx"][[1, 2, 3]].any() and not np.signbit(got["dx"][[1, 2, 3]]).any()
    if p == 0.0:                                                           # the gradients of the batch without them
        ok = [0, 4]
        small = dict(c, B=2, n=c["n"][ok], x=c["x"][ok], d_pred=c["d_pred"][ok])
        fwd2 = run_forward(small, p)
        got2 = run_backward(small, fwd2, p)
        assert same_bits(fwd2["pred"], fwd["pred"][ok]) and same_bits(got2["dx"], got["dx"][ok])
        for k in GRADS:
            assert same_bits(got2[k], got[k]), k


def test_a_batch_without_an_ok_utterance():
    c = make_inputs(2, 3, 4, 64, [0, 9], seed=4)
    want_f, want_b = ref_both(c, 0.5, 11)
    fwd = run_forward(c, 0.5)
    check_forward(fwd, want_f)
    got = run_backward(c, fwd, 0.5)
    check_backward(got, want_b)
    assert all(not v.any() for v in got.values())


# ---------------------------------------------------------------------------------------------------------------- the module

def module_for(c, dropout):
    from b2s_hip import predictor
    m = predictor.VariancePredictor(c["D"], c["F"], dropout=dropout, eps=EPS).to(DEV)
    with torch.no_grad():
        for t, k in zip(m.parameters_in_order(), NAMES):
            t.copy_(dev(c[k], np.float32).reshape(t.shape))
    return m


def test_the_module_through_autograd_has_the_gradients_of_the_call():
    B, S, D, F, p, seed = 3, 33, 36, 64, 0.5, 11
    c = case(B, S, D, F)
    want_f, want_b = reference(B, S, D, F, p, seed)
    m = module_for(c, p).train()
    assert sorted(m.state_dict()) == sorted("%s.%s" % (mod, k) for mod in ("conv1", "norm1", "conv2", "norm2", "linear")
                                            for k in ("weight", "bias"))
    x = dev(c["x"], np.float32).requires_grad_(True)
    out = m(x, c["n"].copy(), seed=seed)
    assert sorted(out) == ["prediction", "status"] and out["status"].cpu().tolist() == [0, 0, 0]
    assert same_bits(out["prediction"].detach().cpu().numpy(), want_f["pred"])
    out["prediction"].backward(dev(c["d_pred"], np.float32))
    assert same_bits(x.grad.cpu().numpy(), want_b["dx"])
    fwd = run_forward(c, p, seed)
    call = run_backward(c, fwd, p, seed)
    for t, k in zip(m.parameters_in_order(), GRADS):
        assert same_bits(t.grad.cpu().numpy().reshape(call[k].shape), call[k]), k
    # only x: the parameter gradients are not computed
    m.zero_grad(set_to_none=True)
    for t in m.parameters():
        t.requires_grad_(False)
    x2 = dev(c["x"], np.float32).requires_grad_(True)
    m(x2, c["n"].copy(), seed=seed)["prediction"].backward(dev(c["d_pred"], np.float32))
    assert same_bits(x2.grad.cpu().numpy(), want_b["dx"]) and all(t.grad is None for t in m.parameters())


def test_eval_ignores_the_seed_and_drops_nothing():
    B, S, D, F = 3, 33, 36, 64
    c = case(B, S, D, F)
    m = module_for(c, 0.5).eval()
    x = dev(c["x"], np.float32)
    with torch.no_grad():
        a, b = m(x, c["n"].copy(), seed=1)["prediction"], m(x, c["n"].copy(), seed=2)["prediction"]
    assert same_bits(a.cpu().numpy(), b.cpu().numpy())
    assert same_bits(a.cpu().numpy(), reference(B, S, D, F, 0.0)[0]["pred"])
    from b2s_hip import B2SError
    with pytest.raises(B2SError, match=r"failed for utterances \[1\]"):
        m(x, [3, 99, 1])
    out = m(x, [3, 99, 1], check_status=False)
    assert out["status"].cpu().tolist() == [0, 2, 0] and not out["prediction"][1].any()


def test_the_prediction_feeds_expand_through_durations_from_prediction():
    from b2s_hip import predictor, variance
    B, S, D, F = 3, 33, 36, 64
    c = case(B, S, D, F)
    m = module_for(c, 0.5).eval()
    x = dev(c["x"], np.float32)
    with torch.no_grad():
        pred = m(x, c["n"].copy())["prediction"]
    dur = predictor.durations_from_prediction(pred + 1.0, c["n"].copy(), alpha=1.3, max_frames=7)
    assert dur.is_cuda and dur.dtype == torch.int32                        # no copy to the host on the way
    want = R.durations_from_prediction(pred.cpu().numpy() + np.float32(1.0), c["n"], 1.3, 7)
    scaled = (np.exp((pred.cpu().numpy() + np.float32(1.0)).astype(np.float64)) - 1.0) * 1.3
    clear = np.abs(scaled - np.floor(scaled) - 0.5) > 0.01
    assert np.array_equal(dur.cpu().numpy()[clear], want[clear]) and int(dur.sum()) > 0
    out = variance.expand(x, dur, c["n"].copy())
    assert out["frame_lengths"] == dur.sum(dim=1).cpu().tolist()
    assert int(out["frames"].shape[0]) == int(dur.sum()) and out["status"].cpu().tolist() == [0, 0, 0]
