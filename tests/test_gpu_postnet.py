"""The postnet segment (b2s_postnet_forward / b2s_postnet_backward, reached through m.postnet(x, lengths)) per element against the float64
restatement tests/postnet_ref.py, at the shapes where its kernels change path (postnet_ref.CASES): the vectorised BatchNorm kernels' channel and row
clamps, the BatchNorm column sums from the three GEMM kernels' epilogues, the backward-data conv with the row-length mask, dropout regenerated in
the backward, the fused residual add, eval mode with non-trivial running statistics, and the one-pass batch variance on inputs that are not zero-mean.

fp32 is held to the project's fp32 bars against plain float64; bf16 to the bf16 bars against the restatement ROUNDED where the engine stores bf16
(same operands: accumulation order and one-ulp rounding flips remain).  tests/test_postnet_ref_host.py checks the checker on the CPU.
Every test prints what it measured; with B2S_TEST_RECORD_DIR set, the worst value per tensor kind goes to r13_postnet_parity.json there
(committed copy: profiles/)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import b2s_oracle as O                     # checker only
from oracle import rng as Rn
from oracle import synth, make_config
from gpu_util import DEV, bf16_round
from test_gpu_model import build
from test_gpu_dropout_parity import site_info
import postnet_ref as R

RECORD = "r13_postnet_parity.json"


def record(tag, bf16, ex):
    """worst error per tensor kind, in the unit of its bar (fp32: max |err|, gradients / max(1, ||ref||_2); bf16: max |err| / max |ref|)."""
    worst = {}
    for k, (over, err) in ex.items():
        kind = R.kind_of(k)
        if kind == "nbt":
            continue
        bar = {"out": R.BAR16_OUT, "grad": R.BAR16_GRAD, "stat": R.BAR16_STAT}[kind] if bf16 else {"out": R.BAR_ACT, "grad": R.BAR_GRAD, "stat": R.BAR_STAT}[kind]
        worst[kind] = max(worst.get(kind, 0.0), over * bar)
    print("%s: " % tag + ", ".join("%s %.2e" % kv for kv in sorted(worst.items())))
    if os.environ.get("B2S_GEMM256_MIN_M"):
        return worst                                    # (the forced-kernel re-run is not what the committed record describes)
    out_dir = os.environ.get("B2S_TEST_RECORD_DIR")
    if not out_dir:
        return worst
    try:
        os.makedirs(out_dir, exist_ok=True)
        path = os.path.join(out_dir, RECORD)
        data = json.load(open(path)) if os.path.exists(path) else {}
        data.setdefault("tests", {})[tag] = worst
        if not tag.startswith("beyond"):
            w = data.setdefault("worst", {}).setdefault("bf16" if bf16 else "fp32", {})
            for k, v in worst.items():
                w[k] = max(w.get(k, 0.0), v)
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)
    except OSError:
        pass
    return worst


def run_hip(over, x, lens, go, compute_dtype="fp32", train=True, fuse=False, state_edit=None, backward=True):
    """m.postnet(x, lens) (+ one backward) on the device -> (the compared tensors by name, P = the state the model was loaded with, cfg, seed)."""
    m, cfg, st, hp = build(over, compute_dtype=compute_dtype, state_edit=state_edit)
    pn = m.postnet
    pn.train() if train else pn.eval()
    xd = x.to(DEV).requires_grad_(backward)
    with torch.set_grad_enabled(backward):
        out = pn(xd, lens.to(DEV), _fuse_add=fuse)
    got = {"out": out.detach().cpu()}
    if backward:
        out.backward(go.to(DEV))
    torch.cuda.synchronize()
    if backward:
        got["x.grad"] = xd.grad.cpu()
        for n, p in pn.named_parameters():
            got[n + ".grad"] = p.grad.detach().cpu()
    for k, v in pn.state_dict().items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            got[k] = v.detach().cpu()
    seed = m.engine().seeds_used.get("postnet")
    return got, O.to_torch_state(st), cfg, seed


def check(tag, got, ref, bf16=False, only=None):
    ex = R.excess(got, {k: v for k, v in ref.items() if only is None or R.kind_of(k) in only}, bf16)
    record(tag, bf16, ex)
    bad = {k: v for k, v in ex.items() if not v[0] <= 1.0}
    assert not bad, (tag, bad)
    return ex


def padded(x, lens):
    return torch.arange(x.shape[1])[None, :] >= lens[:, None]


@pytest.mark.parametrize("case", list(R.CASES))
def test_postnet_train_fp32_vs_fp64(case):
    """Dropout off, every compared tensor at the fp32 bars.  Case H (M = 2 rows) is why the batch variance of up to 64 rows is taken two-pass: with
    the one-pass fp32 variance sum(y^2) / M - mean^2 its layer-2 running_var was 1.61e-5 from float64 (bar 1e-5) -- two rows put any |mean| / std on a
    channel (152 at layer 0) and channels whose variance is below eps turn the variance error into an error of xhat, which the next layers inherit."""
    x, lens, go = R.case_inputs(case)
    bwd = case != "H"                       # (M = 2: the BatchNorm gradient of two points is an exact cancellation, not a parity case)
    got, P, cfg, _ = run_hip(R.case_over(case), x, lens, go, backward=bwd)
    ref = R.step(P, cfg, x, lens, go)
    check("fp32/%s" % case, got, ref, only=None if bwd else ("out", "stat", "nbt"))
    if bwd:
        assert not got["x.grad"][padded(x, lens)].any()


@pytest.mark.parametrize("case", ["A", "B", "D", "F", "I", "J", "K"])
def test_postnet_train_bf16_vs_rounded_fp64(case):
    """B and F take the 256-row kernel (fast and generic epilogue), the others the 128-row kernel; J and K sit either side of the two-pass variance."""
    x, lens, go = R.case_inputs(case)
    got, P, cfg, _ = run_hip(R.case_over(case), x, lens, go, compute_dtype="bf16")
    check("bf16/%s" % case, got, R.step(P, cfg, x, lens, go, round=bf16_round), bf16=True)
    assert not got["x.grad"][padded(x, lens)].any()


@pytest.mark.parametrize("nb", ["3", "4"])
def test_postnet_256_row_tile_kernel_forced(nb):
    """B2S_GEMM256_MIN_M=1 sends every conv of the 16-bit tests of this file through the 256-row tile kernel, both tile widths (as
    test_gpu_ops.py::test_gemm_256_tile_kernel_all_forms does): one child pytest process at a time."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, B2S_GEMM256_MIN_M="1", B2S_GEMM256_NB=nb)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "tests/test_gpu_postnet.py", "-k", "bf16"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]


@pytest.mark.parametrize("dtype,case", [("fp32", "B"), ("fp32", "E"), ("bf16", "B")])
def test_postnet_dropout_on_under_device_masks(dtype, case):
    """decoder_dropout_rate = 0.5: the restatement takes the engine's masks, in the forward and again in the backward."""
    x, lens, go = R.case_inputs(case)
    got, P, cfg, seed = run_hip(R.case_over(case, dropout=0.5), x, lens, go, compute_dtype=dtype)
    src = Rn.DeviceMasks({"postnet": seed}, site_info)
    rnd = bf16_round if dtype == "bf16" else None
    ref = R.step(P, cfg, x, lens, go, masks=src, round=rnd)
    assert len(src.calls) == cfg.n_postnet_layer
    check("%s/%s dropout" % (dtype, case), got, ref, bf16=dtype == "bf16")
    assert not got["x.grad"][padded(x, lens)].any()
    # the dropout really was on: the dropout-off output is more than 100 bars away
    off = R.step(P, cfg, x, lens, go, round=rnd)
    ex = R.excess(got, {k: off[k] for k in ("out", "x.grad")}, dtype == "bf16")
    print("distance from the dropout-off result, in bars: out %.0f, x.grad %.0f" % (ex["out"][0], ex["x.grad"][0]))
    assert ex["out"][0] > 100.0, ex


def _eval_stats(st):
    g = np.random.default_rng(99)
    for k in st:
        if k.startswith("postnet.") and k.endswith("running_mean"):
            st[k] = (0.5 * g.standard_normal(st[k].shape)).astype(np.float32)
        elif k.startswith("postnet.") and k.endswith("running_var"):
            st[k] = g.uniform(0.1, 3.0, st[k].shape).astype(np.float32)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", ["A", "F"])
def test_postnet_eval_running_statistics(case, dtype):
    x, lens, go = R.case_inputs(case)
    got, P, cfg, _ = run_hip(R.case_over(case), x, lens, go, compute_dtype=dtype, train=False, state_edit=_eval_stats, backward=False)
    ref = R.forward(P, cfg, x, lens, train=False, round=bf16_round if dtype == "bf16" else None)
    assert not ref["bn_state"]
    check("%s/%s eval" % (dtype, case), got, {"out": ref["out"]}, bf16=dtype == "bf16")
    for k, v in got.items():                                  # statistics unchanged bit for bit
        if k != "out":
            assert torch.equal(v, P["postnet." + k]), k


def test_postnet_fuse_add():
    """_fuse_add=True: out = postnet(x) + x, x.grad = d_inputs + grad_out."""
    x, lens, go = R.case_inputs("B")
    got, P, cfg, _ = run_hip(R.case_over("B"), x, lens, go, fuse=True)
    ref = R.step(P, cfg, x, lens, go, add_inputs=True)
    ref["x.grad"] = ref["x.grad"] + go.double()
    check("fp32/B fuse_add", got, ref)
    pad = padded(x, lens)
    assert torch.equal(got["x.grad"][pad], go[pad])


@pytest.mark.parametrize("name", list(R.OFFSET_INPUTS))
def test_postnet_nonzero_mean_inputs(name):
    """The batch variance is one-pass fp32, sum(y^2) / M - mean^2 (k_bn_apply_v from the GEMM epilogue's column sums), and real mels are not
    zero-mean.  Inputs x = c + s N(0, 1) over the 280 rows of case B (postnet_ref.OFFSET_INPUTS); the worst channel |mean| / std of the layer-0
    conv output is a condition on the input.  "mel-like" (c = 0.55, s = 0.58, ratio in [0.3, 4]) and "offset" (ratio in [6, 10]) are held to the full
    fp32 bars.  "beyond" (ratio in [28, 36]) only has to stay finite with a non-negative variance; its errors are printed and recorded
    (DESIGN.md section (a))."""
    cfg0 = make_config(R.case_over("B"))
    P0 = O.to_torch_state(synth.synthetic_state(cfg0, 1234))
    x, lens, go, band, (c, s) = R.offset_input(name, P0, cfg0)
    got, P, cfg, _ = run_hip(R.case_over("B"), x, lens, go)
    ref = R.step(P, cfg, x, lens, go)
    ratio = R.channel_ratio(R.forward(P, cfg, x, lens)["y"][0])
    print("%s: c = %.3f, s = %.2f, worst channel |mean| / std of the layer-0 conv output %.2f" % (name, c, s, ratio))
    assert band[0] <= ratio <= band[1], (name, ratio, band)
    if name != "beyond":
        check("fp32/B %s" % name, got, ref)
        return
    ex = R.excess(got, ref)
    record("beyond (|mean| / std = %.0f)" % ratio, False, ex)
    for k, v in got.items():
        assert torch.isfinite(v.double()).all(), k
    # running_var = 0.9 old + 0.1 var M / (M - 1) with var >= 0 (so rstd <= 1 / sqrt(eps)): a negative one-pass variance that was not clamped
    # would show as running_var < 0.9 old (one fp32 rounding of a value near 1 allowed)
    M = x.shape[0] * x.shape[1]
    for i in range(cfg.n_postnet_layer):
        q = "batchnorm_layers.%d." % i
        rv, old = got[q + "running_var"].double(), P["postnet." + q + "running_var"].double()
        assert (rv >= 0).all()
        var = (rv - 0.9 * old) / (0.1 * M / (M - 1.0))
        assert float(var.min()) >= -1e-5 * float(rv.max()), (i, float(var.min()))
        rstd = 1.0 / torch.sqrt(var.clamp(min=0.0) + R.EPS)
        assert float(rstd.max()) <= 1.0 / R.EPS ** 0.5


def test_postnet_single_row_training_batch_is_refused():
    """B T = 1 in training mode has no variance (torch: "Expected more than 1 value per channel when training"): refused before any launch,
    running statistics untouched; eval mode with one row works."""
    from b2s_hip.lib import B2SError
    m, cfg, st, hp = build(R.case_over("A"))
    pn = m.postnet
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 1, cfg.num_mels, generator=g)
    lens = torch.tensor([1])
    before = {k: v.detach().cpu().clone() for k, v in pn.state_dict().items()}
    pn.train()
    with pytest.raises(B2SError, match="more than 1 value per channel"):
        pn(x.to(DEV), lens.to(DEV))
    torch.cuda.synchronize()
    for k, v in pn.state_dict().items():
        assert torch.equal(v.cpu(), before[k]), k
    assert int(pn.batchnorm_layers[0].num_batches_tracked) == 3
    pn.eval()
    with torch.no_grad():
        out = pn(x.to(DEV), lens.to(DEV)).cpu()
    ref = R.forward(O.to_torch_state(st), cfg, x, lens, train=False)["out"]
    err = float((out.double() - ref).abs().max())
    print("one row, eval mode: max |err| = %.2e" % err)
    assert err <= R.BAR_ACT
