"""CPU checks of tests/postnet_ref.py, the float64 restatement tests/test_gpu_postnet.py compares the HIP postnet with: it equals the
oracle (forward, running statistics, and its hand-written backward equals torch autograd of the oracle), the bars tell six deliberately
wrong references from the right one, the mean-offset inputs land in their bands, and the torch-fp32 oracle alone meets every fp32 bar."""
import pytest
import torch

from oracle import b2s_oracle as O                     # checker only
from oracle import synth, make_config
import postnet_ref as R

_MEMO = {}


def setup(case, dtype=torch.float64):
    """(cfg, state dict as torch tensors of `dtype`, x, lengths, grad_out) of a case."""
    if case not in _MEMO:
        cfg = make_config(R.case_over(case))
        _MEMO[case] = (cfg, synth.synthetic_state(cfg, 1234))
    cfg, st = _MEMO[case]
    P = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in O.to_torch_state(st).items()}
    x, lens, go = R.case_inputs(case)
    return cfg, P, x, lens, go


def oracle_step(P, cfg, x, lens, go, dtype):
    """O.postnet_forward + torch autograd in `dtype` -> the tensors the GPU test compares, as float64."""
    names = [n for n in P if n.startswith("postnet.") and O.is_parameter(n)]
    Pg = dict(P)
    for n in names:
        Pg[n] = P[n].clone().requires_grad_(True)
    xi = x.to(dtype).clone().requires_grad_(True)
    bn = {}
    out = O.postnet_forward(Pg, cfg, xi, lens, train=True, bn_state=bn)
    gs = torch.autograd.grad(out, [xi] + [Pg[n] for n in names], go.to(dtype))
    res = {"out": out.detach().double(), "x.grad": gs[0].double()}
    for n, g in zip(names, gs[1:]):
        res[n[len("postnet."):] + ".grad"] = g.double()
    for k, v in bn.items():
        res[k[len("postnet."):]] = v.detach().double() if v.is_floating_point() else v
    return res


ref_step = R.step


def excess(got, ref):
    return {k: v[0] for k, v in R.excess(got, ref).items()}


@pytest.mark.parametrize("case", ["A", "B", "E"])
def test_restatement_equals_oracle_fp64(case):
    cfg, P, x, lens, go = setup(case)
    for train in (True, False):
        bn = {}
        with torch.no_grad():
            want = O.postnet_forward(P, cfg, x.double(), lens, train=train, bn_state=bn)
        r = R.forward(P, cfg, x, lens, train=train)
        assert float((r["out"] - want).abs().max()) <= 1e-12
        assert set(r["bn_state"]) == set(bn) and (len(bn) == 3 * cfg.n_postnet_layer if train else not bn)
        for k, v in bn.items():
            if k.endswith("num_batches_tracked"):
                assert int(r["bn_state"][k]) == int(v) == 4
            else:
                assert float((r["bn_state"][k] - v).abs().max()) <= 1e-12, k
    with torch.no_grad():
        want = O.postnet_forward(P, cfg, x.double(), lens, train=True)
    assert float((R.forward(P, cfg, x, lens, add_inputs=True)["out"] - (want + x.double())).abs().max()) <= 1e-12


@pytest.mark.parametrize("case", ["A", "B", "E", "I"])
def test_hand_written_backward_equals_autograd_of_the_oracle(case):
    cfg, P, x, lens, go = setup(case)
    want = oracle_step(P, cfg, x, lens, go, torch.float64)
    got = ref_step(P, cfg, x, lens, go)
    assert set(got) == set(want)
    for k, r in want.items():
        if r.is_floating_point():
            assert float((got[k] - r).abs().max()) <= 1e-10, k
    T = x.shape[1]
    pad = torch.arange(T)[None, :] >= lens[:, None]
    assert not got["x.grad"][pad].any()


def test_rounding_hook_is_straight_through_and_placed_at_the_storage_points():
    """round= is called on the cast input, n weight images, n - 1 activations, n dy and n - 1 du -- nothing else -- and an identity `round` changes
    nothing."""
    cfg, P, x, lens, go = setup("A")
    calls = []

    def ident(t):
        calls.append(tuple(t.shape))
        return t
    a, b = ref_step(P, cfg, x, lens, go, round=ident), ref_step(P, cfg, x, lens, go)
    n = cfg.n_postnet_layer
    assert len(calls) == 1 + n + (n - 1) + n + (n - 1)
    for k, v in b.items():
        assert torch.equal(a[k], v), k
    bf = ref_step(P, cfg, x, lens, go, round=lambda t: t.to(torch.bfloat16))
    assert 1e-4 < float((bf["out"] - b["out"]).abs().max()) < 0.1


@pytest.mark.parametrize("wrong", R.WRONG)
def test_bars_reject_a_wrong_reference(wrong):
    """Test of the test, case B: each deliberately wrong reference moves at least one compared tensor by more than 10 x its bar."""
    cfg, P, x, lens, go = setup("B")
    ex = excess(ref_step(P, cfg, x, lens, go, wrong=wrong), ref_step(P, cfg, x, lens, go))
    k = max(ex, key=ex.get)
    print("%s: worst %s at %.1f x its bar" % (wrong, k, ex[k]))
    assert ex[k] > 10.0, (wrong, ex)


@pytest.mark.parametrize("name", list(R.OFFSET_INPUTS))
def test_offset_inputs_land_in_their_bands(name):
    cfg, P, _, _, _ = setup("B")
    x, lens, go, band, (c, s) = R.offset_input(name, P, cfg)
    ratio = R.channel_ratio(R.forward(P, cfg, x, lens)["y"][0])
    print("%s: c = %.4f, s = %.2f, worst channel |mean| / std of the layer-0 conv output %.2f" % (name, c, s, ratio))
    assert band[0] <= ratio <= band[1], (name, ratio, band)


@pytest.mark.parametrize("case", list(R.CASES) + list(R.OFFSET_INPUTS))
def test_torch_fp32_oracle_meets_every_fp32_bar(case):
    """The reference itself is good enough for the bars: torch fp32 on the CPU against the fp64 restatement, every compared tensor."""
    if case in R.CASES:
        cfg, P, x, lens, go = setup(case)
    else:
        cfg, P, _, _, _ = setup("B")
        x, lens, go = R.offset_input(case, P, cfg)[:3]
    want = ref_step(P, cfg, x, lens, go)
    P32 = {k: (v.float() if v.is_floating_point() else v) for k, v in P.items()}
    ex = excess(oracle_step(P32, cfg, x, lens, go, torch.float32), want)
    if case == "H":         # (two points per channel: the BatchNorm gradient is an exact cancellation, not a parity case)
        ex = {k: v for k, v in ex.items() if not k.endswith(".grad")}
    k = max(ex, key=ex.get)
    print("%s: torch fp32 worst %s at %.3f x its bar" % (case, k, ex[k]))
    assert ex[k] < 1.0, (case, k, ex[k])
