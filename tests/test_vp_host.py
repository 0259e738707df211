"""CPU-only tests of the variance predictor's host side: the exact fmaf of the NumPy restatement (tests/vp_ref.py) against libm, the
C ABI of libb2s_vp.so (declared, exported, bound; every host-side refusal without a GPU), the dropout rule, the restatement against
torch's CPU autograd in fp64 with the fp32 composition as the yardstick, and durations_from_prediction."""
import copy
import ctypes as C
import ctypes.util
import os
import re

import numpy as np
import pytest
import torch

import vp_ref as R
from test_pros_host import dynamic_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = ["b2s_vp_backward", "b2s_vp_dropout_mask", "b2s_vp_forward", "b2s_vp_last_error", "b2s_vp_tape_bytes", "b2s_vp_version",
                "b2s_vp_ws_bytes"]


# ------------------------------------------------------------------------------------------------------------------------ fma32

def fma_triples():
    """At least 10^5 (a, b, c) in four sets of 30000: exponents spread over +-40; c close to -a * b; a * b + c exactly on an fp32
    halfway point; and a * b + c so little below one that the fp64 sum lands on it."""
    rng = np.random.default_rng(20)
    n = 30000

    def spread(k):
        return (rng.standard_normal(k) * np.exp2(rng.integers(-40, 41, size=k))).astype(np.float32)
    a, b, c = [spread(n)], [spread(n)], [spread(n)]
    aa, bb = spread(n), spread(n)
    near = -(aa * bb)                                                      # the rounded product negated, or a neighbour of it
    up = np.nextafter(near, np.float32(np.inf)).astype(np.float32)
    down = np.nextafter(near, np.float32(-np.inf)).astype(np.float32)
    pick = rng.integers(0, 3, size=n)
    a.append(aa), b.append(bb), c.append(np.where(pick == 0, near, np.where(pick == 1, up, down)).astype(np.float32))
    # c = M * 2^25 has an ulp of 2^25; a * b = odd * 2^24 puts the sum exactly between two fp32
    scale = np.exp2(rng.integers(-30, 31, size=n))
    big = rng.integers(1 << 23, 1 << 24, size=n).astype(np.float64) * 2.0 ** 25
    odd = (2 * rng.integers(0, 4, size=n) + 1).astype(np.float64)
    a.append((4096.0 * odd * scale).astype(np.float32)), b.append(np.full(n, 4096.0, np.float32)), c.append((big * scale).astype(np.float32))
    # (1 + t)(1 - t) = 1 - t^2 with t = i * 2^-23: the product is 2^24 * (1 - i^2 * 2^-46), which the fp64 sum with c rounds to 2^24
    t = rng.integers(1, 1000, size=n).astype(np.float64) * 2.0 ** -23
    big = rng.integers(1 << 23, 1 << 24, size=n).astype(np.float64) * 2.0 ** 25
    a.append((4096.0 * (1.0 + t) * scale).astype(np.float32)), b.append((4096.0 * (1.0 - t)).astype(np.float32))
    c.append((big * scale).astype(np.float32))
    return np.concatenate(a), np.concatenate(b), np.concatenate(c)


def test_fma32_is_libm_fmaf_bit_for_bit():
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype = C.c_float
    libm.fmaf.argtypes = [C.c_float, C.c_float, C.c_float]
    a, b, c = fma_triples()
    assert len(a) >= 100000
    got = R.fma32(a, b, c)
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=np.float32)
    assert np.all(np.isfinite(want))
    assert np.array_equal(R.bits(got), R.bits(want))
    # the sets are sharp: a product rounded before the sum, and a sum rounded to fp64 before fp32, each differ from fmaf on them
    assert not np.array_equal(R.bits(a * b + c), R.bits(want))
    twice = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert np.count_nonzero(R.bits(twice) != R.bits(want)) > 1000
    assert np.count_nonzero(np.abs(want[30000:60000]) < 1e-3 * np.abs(c[30000:60000])) > 10000       # cancellation


# --------------------------------------------------------------------------------------------------------------------- the C ABI

def test_header_exports_and_prototypes_are_the_same_names():
    from b2s_hip import cbind, predictor
    l = predictor.load()
    header = open(os.path.join(ROOT, "include", "b2s_vp.h")).read()
    declared = sorted(set(re.findall(r"\b(b2s_vp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert declared == predictor.EXPORTS == sorted(predictor._PROTOS) == ENTRY_POINTS
    assert sorted(n for n in dynamic_symbols(predictor.LIB_PATH) if n.startswith("b2s_")) == ENTRY_POINTS       # exactly these
    assert len(ENTRY_POINTS) == 7
    assert l.b2s_vp_version() >= 100
    assert predictor.LIB_PATH.endswith("few-shot-transformer-tts_amd/libb2s_vp.so")
    assert predictor.B2SError is cbind.B2SError
    assert (predictor.OK, predictor.EMPTY, predictor.FAILED) == (R.OK, R.EMPTY, R.FAILED) == (cbind.OK, cbind.EMPTY, cbind.FAILED)
    for name, value in (("OK", "0"), ("EMPTY", "1"), ("FAILED", "2"), ("MAX_S", "1024"), ("MAX_D", "1024")):
        assert re.search(r"#define B2S_VP_%s %s(\s|$)" % (name, value), header), name
    assert (predictor.MAX_S, predictor.MAX_D, predictor.FILTERS) == (R.MAX_S, R.MAX_D, R.FILTERS) == (1024, 1024, (64, 128, 256, 512))
    assert "`libb2s_vp.so`, 7 entry points" in open(os.path.join(ROOT, "README.md")).read()


def test_the_other_libraries_do_not_grow():
    from b2s_hip import durations, f0, lib, mcd, metrics, prosody, variance, vocoder
    for mod in (lib, vocoder, metrics, mcd, f0, durations, prosody, variance):
        assert not [n for n in mod.EXPORTS if n.startswith("b2s_vp")]


def test_workspace_and_tape_formulas():
    from b2s_hip import predictor
    l = predictor.load()
    a = R.align256
    for B, S, D, F in ((1, 1, 4, 64), (3, 5, 8, 128), (64, 128, 768, 256), (5, 257, 68, 512), (65535, 1, 4, 64)):
        want = 256 + 2 * a(3 * D * F * 4) + 2 * a(3 * F * F * 4) + 3 * a(B * S * F * 4) + a((5 * F + 1) * B * 4)
        assert l.b2s_vp_ws_bytes(B, S, D, F) == want == R.ws_bytes(B, S, D, F)
        assert l.b2s_vp_tape_bytes(B, S, F) == 5 * a(B * S * F * 4) + 2 * a(B * S * 4) == R.tape_bytes(B, S, F)
    assert 2 * a(3 * 768 * 256 * 4) // 2 == 2359296                        # the repacked W1 of the benchmark: 2.4 MB


def test_host_side_refusals_come_back_as_messages_without_a_gpu():
    from b2s_hip import B2SError, predictor
    l = predictor.load()

    def err():
        return l.b2s_vp_last_error().decode()
    d = C.c_void_p(4096)                 # never dereferenced: every call below fails its checks before a launch
    odd = C.c_void_p(4096 + 8)           # 8-byte aligned only
    big = 1 << 40

    for bad in (0, -1):
        assert l.b2s_vp_ws_bytes(bad, 8, 8, 64) == 0 and "B must be > 0 (got %d)" % bad in err()
        assert l.b2s_vp_tape_bytes(bad, 8, 64) == 0 and "B must be > 0 (got %d)" % bad in err()
    assert l.b2s_vp_ws_bytes(65536, 8, 8, 64) == 0 and "split the batch" in err()
    for bad in (0, 1025):
        assert l.b2s_vp_ws_bytes(2, bad, 8, 64) == 0 and "S must be in 1..1024 (got %d)" % bad in err()
        assert l.b2s_vp_tape_bytes(2, bad, 64) == 0 and "S must be in 1..1024 (got %d)" % bad in err()
    for bad in (0, 6, 1028, -4):
        assert l.b2s_vp_ws_bytes(2, 8, bad, 64) == 0 and "D must be a multiple of 4 in 4..1024 (got %d)" % bad in err()
    for bad in (0, 32, 96, 192, 1024, -64):
        assert l.b2s_vp_ws_bytes(2, 8, 8, bad) == 0 and "F must be 64, 128, 256 or 512 (got %d)" % bad in err()
        assert l.b2s_vp_tape_bytes(2, 8, bad) == 0 and "F must be 64, 128, 256 or 512 (got %d)" % bad in err()
    assert l.b2s_vp_ws_bytes(65535, 1024, 1024, 64) == 0 and "sizes past one call" in err()
    assert l.b2s_vp_ws_bytes(65535, 1024, 4, 512) == 0 and "sizes past one call" in err()
    assert l.b2s_vp_tape_bytes(65535, 1024, 512) == 0 and "sizes past one call" in err()
    assert l.b2s_vp_ws_bytes(2048, 1024, 1024, 512) > 0                    # exactly 2^31 elements
    with pytest.raises(B2SError, match="F must be 64, 128, 256 or 512"):
        predictor.workspace(l.b2s_vp_ws_bytes(2, 8, 8, 100), "cpu")

    def fwd(x=d, n=d, params=None, eps=1e-5, p=0.0, B=2, S=8, D=8, F=64, pred=d, status=d, tape=d, ws=d, ws_bytes=big):
        params = [d] * 10 if params is None else params
        return l.b2s_vp_forward(x, n, *params, eps, p, 1, B, S, D, F, pred, status, tape, ws, ws_bytes, None)

    def bwd(x=d, n=d, params=None, tape=d, d_pred=d, p=0.0, B=2, S=8, D=8, F=64, dx=d, grads=None, ws=d, ws_bytes=big):
        params = [d] * 10 if params is None else params
        grads = [d] * 10 if grads is None else grads
        return l.b2s_vp_backward(x, n, *params, tape, d_pred, p, 1, B, S, D, F, dx, *grads, ws, ws_bytes, None)

    for call in (fwd, bwd):
        assert call(F=96) == 1 and "F must be 64, 128, 256 or 512 (got 96)" in err()
        assert call(D=6) == 1 and "D must be a multiple of 4 in 4..1024 (got 6)" in err()
        assert call(B=0) == 1 and "B must be > 0" in err()
        assert call(B=65536) == 1 and "split the batch" in err()
        assert call(S=1025) == 1 and "S must be in 1..1024" in err()
        assert call(B=65535, S=1024, D=1024) == 1 and "sizes past one call" in err()
        for bad in (-0.1, 1.0, 1.5, float("nan")):
            assert call(p=bad) == 1 and "p must be in [0, 1)" in err()
        assert call(x=None) == 1 and "is NULL" in err()
        assert call(n=None) == 1 and "is NULL" in err()
        for i in range(10):
            assert call(params=[None if k == i else d for k in range(10)]) == 1 and "a parameter is NULL" in err()
        assert call(x=odd) == 1 and "16-byte aligned" in err()
        assert call(tape=odd) == 1 and "16-byte aligned" in err()
        assert call(ws=None) == 1 and "workspace of 0 bytes" in err()
        need = l.b2s_vp_ws_bytes(2, 8, 8, 64)
        assert call(ws_bytes=need - 1) == 1 and "workspace of %d bytes, %d needed" % (need - 1, need) in err()
    assert fwd(pred=None) == 1 and "is NULL" in err()
    assert fwd(status=None) == 1 and "is NULL" in err()
    assert fwd(eps=-1.0) == 1 and "eps must be >= 0" in err()
    assert bwd(tape=None) == 1 and "is NULL" in err()
    assert bwd(d_pred=None) == 1 and "is NULL" in err()
    assert bwd(dx=odd) == 1 and "16-byte aligned" in err()
    # the NULL mismatch: the ten parameter gradients come together
    for i in range(10):
        assert bwd(grads=[None if k == i else d for k in range(10)]) == 1 and "NULL together or not at all (9 are there)" in err()
    assert bwd(grads=[d] + [None] * 9) == 1 and "(1 are there)" in err()
    assert bwd(grads=[None] * 10, dx=None) == 1 and "nothing to compute" in err()

    def msk(p=0.5, site=1, B=2, S=8, F=64, out=d):
        return l.b2s_vp_dropout_mask(p, 1, site, B, S, F, out, None)
    assert msk(p=1.0) == 1 and "p must be in [0, 1)" in err()
    for bad in (0, 3):
        assert msk(site=bad) == 1 and "site must be 1 or 2 (got %d)" % bad in err()
    assert msk(F=100) == 1 and "F must be" in err()
    assert msk(out=None) == 1 and "out_bytes is NULL" in err()


def test_python_side_refusals():
    from b2s_hip import B2SError, predictor
    with pytest.raises(B2SError, match="D must be a multiple of 4"):
        predictor.VariancePredictor(10)
    with pytest.raises(B2SError, match="F must be 64, 128, 256 or 512"):
        predictor.VariancePredictor(8, 100)
    with pytest.raises(B2SError, match=r"p must be in \[0, 1\)"):
        predictor.VariancePredictor(8, 64, dropout=1.0)
    with pytest.raises(B2SError, match="on the GPU"):
        predictor.predict(torch.zeros(1, 2, 8), [2], [torch.zeros(1)] * 10)
    m = predictor.VariancePredictor(8, 64)
    assert sorted(m.state_dict()) == sorted(
        "%s.%s" % (mod, k) for mod in ("conv1", "norm1", "conv2", "norm2", "linear") for k in ("weight", "bias"))
    assert [tuple(t.shape) for t in m.parameters_in_order()] == [(64, 8, 3), (64,), (64,), (64,), (64, 64, 3), (64,), (64,), (64,),
                                                                 (1, 64), (1,)]


# --------------------------------------------------------------------------------------------------------------------- the mask

def test_mask_restatement():
    assert R.mask(0.0, 5, 1, 2, 3, 64).all()                               # p = 0 keeps all
    N = 1 << 20
    k = R.mask(0.5, 1234, 1, 16, 256, 256)
    assert k.size == N
    assert abs(k.mean() - 0.5) <= 4 * np.sqrt(0.25 / N)                    # 4 binomial standard deviations
    other_site, other_seed = R.mask(0.5, 1234, 2, 16, 256, 256), R.mask(0.5, 1235, 1, 16, 256, 256)
    hi_seed = R.mask(0.5, 1234 + (1 << 32), 1, 16, 256, 256)
    for o in (other_site, other_seed, hi_seed):
        assert 0.4 < np.mean(o != k) < 0.6                                 # as different as two independent masks
    assert R.drop_constants(0.5, 0, 1)[1:] == (1 << 31, np.float32(2.0))
    assert R.drop_constants(0.25, 0, 1)[1] == 1 << 30
    assert int(R.lowbias32(0)) == 0 and len(set(int(v) for v in R.lowbias32(np.arange(1000)))) == 1000       # a bijection


# ------------------------------------------------------------------------------------- the restatement against torch on the CPU

def test_restatement_against_torch_fp64_with_the_fp32_composition_as_yardstick(capsys):
    """B = 3, S = 65, D = 68, F = 64, random normal data, the same masks on both sides.  Both the restatement and torch's fp32
    composition are fp32 evaluations of one function in different summation orders; each one's relative L2 error to torch's fp64
    result is measured per tensor, and the restatement's must be at most 4x the composition's (which must not be zero)."""
    from b2s_hip import predictor
    B, S, D, F, p, seed = 3, 65, 68, 64, 0.5, 77
    rng = np.random.default_rng(5)
    torch.manual_seed(5)
    m32 = predictor.VariancePredictor(D, F, dropout=p)
    with torch.no_grad():
        for norm in (m32.norm1, m32.norm2):
            norm.weight.copy_(1.0 + 0.2 * torch.randn(F))
            norm.bias.copy_(0.2 * torch.randn(F))
    m32.train()
    m64 = copy.deepcopy(m32).double()
    x = rng.standard_normal((B, S, D)).astype(np.float32)
    n = np.array([S, S // 2, 1], np.int32)
    d_pred = rng.standard_normal((B, S)).astype(np.float32)
    keep = (R.mask(p, seed, 1, B, S, F), R.mask(p, seed, 2, B, S, F))

    def torch_side(m, dtype):
        xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
        pred = m.reference_forward(xt, torch.from_numpy(n), keep=[torch.from_numpy(k) for k in keep])
        pred.backward(torch.from_numpy(d_pred).to(dtype))
        out = {"pred": pred.detach(), "dx": xt.grad}
        for name, t in zip(("dW1", "db1", "dg1", "dbe1", "dW2", "db2", "dg2", "dbe2", "dwl", "dbl"), m.parameters_in_order()):
            out[name] = t.grad.reshape(-1) if name == "dwl" else t.grad
        return {k: v.double().numpy() for k, v in out.items()}
    t64, t32 = torch_side(m64, torch.float64), torch_side(m32, torch.float32)
    P = {k: t.detach().numpy().reshape(-1) if k == "wl" else t.detach().numpy()
         for k, t in zip(predictor.PARAM_NAMES, m32.parameters_in_order())}
    fwd = R.forward(x, n, P, m32.eps, p=p, seed=seed, masks=keep)
    assert fwd["status"].tolist() == [0, 0, 0]
    mine = dict(R.backward(x, n, P, fwd, d_pred), pred=fwd["pred"])

    def rel(a, truth):
        return float(np.linalg.norm((np.asarray(a, np.float64) - truth).ravel()) / np.linalg.norm(truth.ravel()))
    lines, bad = [], []
    for k in ("pred", "dx", "dW1", "db1", "dg1", "dbe1", "dW2", "db2", "dg2", "dbe2", "dwl", "dbl"):
        e_mine, e_32 = rel(mine[k], t64[k]), rel(t32[k], t64[k])
        lines.append("%-5s restatement %.3e   fp32 composition %.3e   ratio %.2f" % (k, e_mine, e_32, e_mine / e_32 if e_32 else np.inf))
        if not (e_32 > 0.0 and e_mine <= 4.0 * e_32):
            bad.append(k)
    with capsys.disabled():
        print("\nrelative L2 error to torch fp64 (B=3, S=65, D=68, F=64, p=0.5):\n" + "\n".join(lines))
    assert not bad, "\n".join(lines)


# ---------------------------------------------------------------------------------------------------- durations_from_prediction

def test_durations_from_prediction_equals_the_restatement():
    from b2s_hip import predictor, variance
    rng = np.random.default_rng(9)
    B, S = 4, 50
    n = np.array([50, 17, 0, 1], np.int32)
    for alpha in (0.5, 1.0, 1.3):
        pred = rng.uniform(-2.0, 4.5, size=(B, S)).astype(np.float32)
        pred[0, :4] = [-5.0, 0.0, 9.0, 20.0]                               # the clamp at 0 and at max_frames
        scaled = (np.exp(pred.astype(np.float64)) - 1.0) * alpha
        near = np.abs(scaled - np.floor(scaled) - 0.5) < 0.01
        pred[near] = np.float32(0.0)                                       # away from a .5 boundary
        scaled = (np.exp(pred.astype(np.float64)) - 1.0) * alpha
        assert not (np.abs(scaled - np.floor(scaled) - 0.5) < 0.01).any()
        for max_frames in (60, predictor.DEFAULT_MAX_FRAMES):
            got = predictor.durations_from_prediction(torch.from_numpy(pred), n, alpha=alpha, max_frames=max_frames)
            assert got.dtype == torch.int32 and tuple(got.shape) == (B, S)
            want = R.durations_from_prediction(pred, n, alpha, max_frames)
            assert np.array_equal(got.numpy(), want)
            assert got[0, 0] == 0 and got[0, 1] == 0 and got[0, 3] == max_frames and int(got.max()) <= max_frames
            assert not got[1, 17:].any() and not got[2].any() and not got[3, 1:].any()
            assert int(got.min()) == 0
    assert predictor.DEFAULT_MAX_FRAMES * predictor.MAX_S <= variance.MAX_FRAMES
