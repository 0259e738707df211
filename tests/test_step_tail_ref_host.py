"""CPU checks of tests/step_tail_ref.py, the float64 restatement tests/test_gpu_step_tail.py compares the loss, L2 and fused-Adam kernels with: it
equals the oracle (loss values, autograd gradients, torch.optim.Adam, oracle.adam_step), the bars tell eleven deliberately wrong references from the
right one on the inputs of the GPU test, and the float32 run of the same statements meets every fp32 bar (no bar is tighter than honest fp32)."""
import itertools

import numpy as np
import pytest
import torch

from oracle import b2s_oracle as O                     # checker only
from oracle import synth, make_config, TINY, TINY96
import step_tail_ref as R

_MEMO = {}


def tiny_params(over=TINY):
    """{name: fp32 array} of the parameters of a synthetic state, state_dict order."""
    if over not in _MEMO:
        st = synth.synthetic_state(make_config(over), 1234)
        _MEMO[over] = {n: np.asarray(v) for n, v in st.items() if O.is_parameter(n)}
    return _MEMO[over]


def oracle_loss(case, dtype=torch.float64, w3=None):
    bef, aft, stop, tgt, lens = R.loss_inputs(case)
    cfg = make_config(TINY)
    P = {n: torch.from_numpy(v).to(dtype) for n, v in tiny_params().items()}
    outs = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in (("mel_bef", bef), ("mel_aft", aft), ("stop_logits", stop))}
    res = O.compute_loss(P, cfg, torch.from_numpy(tgt).to(dtype), torch.from_numpy(lens), outs)
    w = (1.0, 1.0, 1.0) if w3 is None else w3
    (w[0] * res["bef_loss"] + w[1] * res["aft_loss"] + w[2] * res["stop_loss"]).backward()
    return res, outs


@pytest.mark.parametrize("case", list(R.LOSS_CASES))
def test_loss_equals_oracle_fp64(case):
    bef, aft, stop, tgt, lens = R.loss_inputs(case)
    res, _ = oracle_loss(case)
    l2 = R.l2_value(tiny_params(), make_config(TINY).reg_weight)
    assert abs(l2 - float(res["l2"])) <= 1e-12 * abs(l2) and l2 > 0
    out, per = R.loss(bef, aft, stop, tgt, lens, l2)
    for i, k in enumerate(("loss", "bef_loss", "aft_loss", "mse_loss", "l2", "stop_loss")):
        want = float(res[k].detach())
        assert abs(out[i] - want) <= 1e-12 * max(1.0, abs(want)), k
    assert out[6] == lens.sum()
    assert np.abs(per - res["aft_losses"].detach().numpy()).max() <= 1e-12 * max(1.0, float(per.max()))


@pytest.mark.parametrize("w3", R.W3)
@pytest.mark.parametrize("case", list(R.LOSS_CASES))
def test_loss_grads_equal_autograd_of_the_oracle(case, w3):
    bef, aft, stop, tgt, lens = R.loss_inputs(case)
    _, outs = oracle_loss(case, w3=w3)
    got = R.loss_grads(bef, aft, stop, tgt, lens, w3)
    for g, k in zip(got, ("mel_bef", "mel_aft", "stop_logits")):
        assert np.abs(g - outs[k].grad.numpy()).max() <= 1e-10, k
    pad = ~R._valid(lens, tgt.shape[1])
    for g in got:
        assert not g[pad].any()
    assert (got[0][bef == tgt] == 0).all() and (bef == tgt)[~pad].sum() > 0 or case == "one-frame"


def test_l2_member_set_is_the_oracles():
    for over in (TINY, TINY96):
        for n in tiny_params(over):
            assert R.l2_member(n) == O.l2_member(n), n
    names = list(tiny_params())
    assert any(R.l2_member(n) for n in names) and any("layer_norm" in n and "weight" in n for n in names)
    g = R.l2_grad(tiny_params(), 0.1, 0.5)
    assert set(g) == {n for n in names if O.l2_member(n)}


def test_adam_equals_torch_adam_and_the_oracle_fp64():
    """Three steps; two param groups: weight_decay = l2 for the members, 0 for the rest."""
    cfg = make_config(TINY)
    names = list(tiny_params())[:40] + ["postnet.conv_layers.0.weight"]
    lr, eps, l2 = 1e-3, cfg.adam_eps, 0.1
    for l2 in (0.1, 0.0):
        cur = {}
        for n in names:
            p, _, _, _ = R.adam_inputs(n, tiny_params()[n].size)
            cur[n] = [p.astype(np.float64), np.zeros(p.size), np.zeros(p.size)]
        tp = {n: torch.nn.Parameter(torch.from_numpy(cur[n][0].copy())) for n in names}
        opt = torch.optim.Adam([{"params": [tp[n] for n in names if R.l2_member(n)], "weight_decay": l2},
                                {"params": [tp[n] for n in names if not R.l2_member(n)], "weight_decay": 0.0}], lr=lr, betas=(0.9, 0.999), eps=eps)
        OP = {n: torch.from_numpy(cur[n][0].copy()) for n in names}
        ostate = {}
        for t in (1, 2, 3):
            grads = {n: R.adam_inputs(n, cur[n][0].size, seed=t)[1].astype(np.float64) for n in names}
            for n in names:
                tp[n].grad = torch.from_numpy(grads[n].copy())
                cur[n] = list(R.adam(cur[n][0], grads[n], cur[n][1], cur[n][2], lr, t, 0.9, 0.999, eps, l2, 1.0, R.l2_member(n)))
            opt.step()
            if l2 == 0.0:
                assert O.learning_rate_schedule(t - 1, cfg) == 1.0 and cfg.max_lr == lr
                O.adam_step(OP, {n: torch.from_numpy(grads[n]) for n in names}, ostate, t - 1, cfg)
        for n in names:
            assert np.abs(cur[n][0] - tp[n].detach().numpy()).max() <= 1e-12, n
            st = opt.state[tp[n]]
            assert np.abs(cur[n][1] - st["exp_avg"].numpy()).max() <= 1e-12 and np.abs(cur[n][2] - st["exp_avg_sq"].numpy()).max() <= 1e-12, n
            if l2 == 0.0:
                assert np.abs(cur[n][0] - OP[n].numpy()).max() <= 1e-12, n


def test_conv_images_are_the_gemm_operands_of_the_conv_and_its_transpose():
    g = torch.Generator().manual_seed(5)
    w = torch.randn(6, 4, 5, generator=g, dtype=torch.float64)
    x, dy = torch.randn(2, 9, 4, generator=g, dtype=torch.float64), torch.randn(2, 9, 6, generator=g, dtype=torch.float64)
    cols = lambda u: torch.cat([torch.nn.functional.pad(u, (0, 0, 2, 2))[:, j:j + u.shape[1]] for j in range(5)], dim=2)       # [B, T, 5 C], tap-major
    y = torch.nn.functional.conv1d(x.transpose(1, 2), w, None, 1, 2).transpose(1, 2)
    dx = torch.nn.functional.conv_transpose1d(dy.transpose(1, 2), w, None, 1, 2).transpose(1, 2)
    fwd, bwd = (torch.from_numpy(a) for a in R.conv_images(w.numpy()))
    assert float((cols(x) @ fwd.T - y).abs().max()) <= 1e-12 and float((cols(dy) @ bwd.T - dx).abs().max()) <= 1e-12
    assert fwd[3, 2 * 4 + 1] == w[3, 1, 2] and bwd[1, (4 - 0) * 6 + 3] == w[3, 1, 0]
    assert np.array_equal(R.bf16_rne(w.numpy()), w.to(torch.float32).to(torch.bfloat16).to(torch.float32).numpy())
    tie = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -8], dtype=np.float32)          # ties go to the even mantissa
    assert np.array_equal(R.bf16_rne(tie), np.array([1.0, 1.0 + 2.0 ** -6, -1.0], dtype=np.float32))


# ----------------------------------------------------------------------------------------------------------------- the test of the test
MUT_CASES = ("golden", "partial-unroll", "many", "mels8")


def _loss_all(case, w3, dtype=np.float64, wrong=None):
    bef, aft, stop, tgt, lens = R.loss_inputs(case)
    out, per = R.loss(bef, aft, stop, tgt, lens, 1e-6, dtype=dtype, wrong=wrong)
    db, da, ds = R.loss_grads(bef, aft, stop, tgt, lens, w3, dtype=dtype, wrong=wrong)
    return {"out": out, "aft_losses": per, "d_bef": db, "d_aft": da, "d_stop": ds, "lens": lens}


def adam_cases():
    return list(itertools.product(R.ADAM_STEPS, R.ADAM_SCALES, (0.0, float(np.float32(5e-9)), float(np.float32(0.1)))))


def adam_excess(got, p, g, m, v, hyper, member):
    """worst (error / bar) of p', m', v' against the float64 restatement."""
    ref = R.adam(p, g, m, v, *hyper, member)
    bars = R.adam_bars(p, g, m, v, *hyper, member)
    worst = []
    for a, r, b in zip(got, ref, bars):
        d = np.abs(np.asarray(a, dtype=np.float64) - r)
        with np.errstate(divide="ignore", invalid="ignore"):
            worst.append(float(np.max(np.where(d == 0, 0.0, d / b))))
    return worst


@pytest.mark.parametrize("wrong", R.WRONG_LOSS)
def test_bars_reject_a_wrong_loss(wrong):
    for case in MUT_CASES:
        ex = {}
        for w3 in R.W3:
            e = R.loss_excess(_loss_all(case, w3, wrong=wrong), _loss_all(case, w3), w3)
            ex.update({(k, w3): v[0] for k, v in e.items()})
        k = max(ex, key=ex.get)
        print("%s / %s: worst %s at %.3g x its bar" % (wrong, case, k[0], ex[k]))
        assert ex[k] > 10.0, (wrong, case, ex)


@pytest.mark.parametrize("wrong", R.WRONG_ADAM)
def test_bars_reject_a_wrong_adam(wrong):
    """step 7, grad_scale 0.5, l2 0.1 on the TINY tensors of the GPU test."""
    hyper = (float(np.float32(0.05)), 7, R.BETA1, R.BETA2, float(np.float32(5e-8)), float(np.float32(0.1)), 0.5)
    mf = R.member_fn(wrong)
    worst = 0.0
    for n, t in tiny_params().items():
        p, g, m, v = R.adam_inputs(n, t.size)
        with np.errstate(invalid="ignore"):              # (v_with_g: a negative v')
            got = R.adam(p, g, m, v, *hyper, mf(n), wrong=None if wrong == "l2_on_layer_norm" else wrong)
        worst = max(worst, max(adam_excess(got, p, g, m, v, hyper, R.l2_member(n))))
    print("%s: worst element at %.3g x its bar" % (wrong, worst))
    assert worst > 10.0, (wrong, worst)


def test_bars_reject_the_unflipped_backward_image():
    """The images are compared bit for bit (through the forward pass on the GPU): any differing element is beyond the bar."""
    n = "postnet.conv_layers.1.weight"
    w = tiny_params()[n]
    (f0, b0), (f1, b1) = R.conv_images(R.bf16_rne(w)), R.conv_images(R.bf16_rne(w), wrong="no_tap_flip")
    assert np.array_equal(f0, f1) and float((b0 != b1).mean()) > 0.7


# ----------------------------------------------------------------------------------------------------------------- honest fp32 meets every bar
@pytest.mark.parametrize("case", list(R.LOSS_CASES))
def test_float32_loss_meets_every_bar(case):
    for w3 in R.W3:
        ex = R.loss_excess(_loss_all(case, w3, dtype=np.float32), _loss_all(case, w3), w3)
        print("%s w3=%s: " % (case, w3) + ", ".join("%s %.2e (%.2f bars)" % (k, v[1], v[0]) for k, v in sorted(ex.items())))
        assert all(v[0] <= 1.0 for v in ex.values()), (case, w3, ex)


def test_measured_bars_are_within_the_projects_scalar_bar():
    assert max(R.BAR_SCALAR, R.BAR_AFT_LOSSES, R.BAR_L2) <= R.CAP_REL and R.BAR_DSTOP <= R.CAP_ABS


@pytest.mark.parametrize("over", [TINY, TINY96], ids=["tiny", "tiny96"])
def test_float32_adam_and_l2_meet_every_bar(over):
    worst = [0.0, 0.0, 0.0]
    for step, gs, l2 in adam_cases():
        hyper = (float(np.float32(1e-3)), step, R.BETA1, R.BETA2, float(np.float32(5e-8)), l2, gs)
        for n, t in tiny_params(over).items():
            p, g, m, v = R.adam_inputs(n, t.size)
            got = R.adam(p, g, m, v, *hyper, R.l2_member(n), dtype=np.float32)
            assert all(a.dtype == np.float32 for a in got)
            worst = [max(a, b) for a, b in zip(worst, adam_excess(got, p, g, m, v, hyper, R.l2_member(n)))]
    print("float32 restatement, worst element in bars: p %.3f, m %.3f, v %.3f" % tuple(worst))
    assert max(worst) <= 1.0, worst
    a32 = np.float32(5e-9) * np.float32(0.5)
    for n, t in tiny_params(over).items():
        if R.l2_member(n):
            p, g, _, _ = R.adam_inputs(n, t.size)
            got = g + a32 * p
            assert got.dtype == np.float32
            ref = g.astype(np.float64) + R.l2_grad({n: p}, float(np.float32(5e-9)), 0.5)[n]
            bar = R.BAR_L2_BWD * R.SLACK * (np.abs(g.astype(np.float64)) + np.abs(float(a32) * p.astype(np.float64)))
            assert (np.abs(got - ref) <= bar).all(), n


@pytest.mark.parametrize("over", [TINY, TINY96], ids=["tiny", "tiny96"])
def test_float32_l2_value_meets_its_bar(over):
    """reg_weight / 2 times the float32 sum of the float32 squares, tensor by tensor (numpy's pairwise sum), against l2_value."""
    P = {n: R.adam_inputs(n, t.size)[0] for n, t in tiny_params(over).items()}
    rw = np.float32(5e-9)
    acc = np.float32(0)
    for n, p in P.items():
        if R.l2_member(n):
            acc = acc + (p * p).sum(dtype=np.float32)
    got, ref = float(acc * (np.float32(0.5) * rw)), R.l2_value(P, float(rw))
    print("float32 l2: rel. error %.2e" % (abs(got - ref) / ref))
    assert abs(got - ref) / ref <= R.BAR_L2
