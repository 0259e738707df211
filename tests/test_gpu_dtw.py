"""The batched GPU FastDTW and MSE-after-DTW metric (b2s_hip.metrics, libb2s_metrics.so) against the fp64 restatement of fastdtw 0.3.4
and the reference's calculate_mse_dtw (tests/dtw_ref.py).

Paths must be identical.  The cost may differ only by the order of the per-cell distance sum (NumPy's ddot), so its gate is 1e-12
relative; on integer-valued inputs every distance is exact and costs must be bit-identical, ties included.  The MSE is fp64 on the
GPU against the reference's fp32 NumPy mean: 1e-5 relative."""
import numpy as np
import pytest
import torch

import dtw_ref as R

pytestmark = pytest.mark.gpu


def _walk(rng, n, dim):
    """Random walk clipped to [-4, 4] like normalised mels."""
    return np.clip(np.cumsum(rng.standard_normal((n, dim)) * 0.3, axis=0), -4, 4).astype(np.float32)


def _warp(rng, a, m, noise=0.1):
    """Time-warped, noisy copy of `a` with m frames."""
    t = np.sort(rng.uniform(0, len(a) - 1, size=m))
    t[0], t[-1] = 0, len(a) - 1
    return np.clip(a[np.round(t).astype(int)] + noise * rng.standard_normal((m, a.shape[1])), -4, 4).astype(np.float32)


def _pad(seqs):
    T, dim = max(len(s) for s in seqs), seqs[0].shape[1]
    out = np.zeros((len(seqs), max(T, 1), dim), np.float32)
    for i, s in enumerate(seqs):
        out[i, :len(s)] = s
    return out


def _check_pairs(xs, ys, radius, exact_cost=False):
    from b2s_hip import metrics
    cost, paths = metrics.dtw_batch(_pad(xs), [len(a) for a in xs], _pad(ys), [len(b) for b in ys], radius=radius, return_paths=True)
    cost = cost.cpu().numpy()
    for b, (a, c) in enumerate(zip(xs, ys)):
        ref_cost, ref_path = R.fastdtw(a, c, radius=radius) if radius else R.dtw(a, c)
        assert [tuple(p) for p in paths[b].tolist()] == ref_path, "pair %d (%d x %d, radius %s): paths differ" % (b, len(a), len(c), radius)
        if exact_cost:
            assert cost[b] == ref_cost, (b, cost[b], ref_cost)
        else:
            assert abs(cost[b] - ref_cost) <= 1e-12 * abs(ref_cost), (b, cost[b], ref_cost)


@pytest.mark.parametrize("dim", [80, 1])
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_fastdtw_paths_and_costs_match_the_restatement(radius, dim):
    rng = np.random.default_rng(100 * radius + dim)
    xs, ys = [], []
    for n, m in ((240, 200), (517, 480), (1100, 1000), (333, 611), (64, 63)):
        a = _walk(rng, n, dim)
        xs.append(a)
        ys.append(_warp(rng, a, m))
    _check_pairs(xs, ys, radius)


def test_exact_dtw_matches_the_restatement():
    rng = np.random.default_rng(7)
    xs = [_walk(rng, n, 80) for n in (300, 120, 5, 1)]
    ys = [_warp(rng, xs[0], 300), _warp(rng, xs[1], 77), _walk(rng, 9, 80), _walk(rng, 4, 80)]
    _check_pairs(xs, ys, None)


@pytest.mark.parametrize("radius", [1, 2, None])
def test_integer_inputs_with_ties_are_bit_identical(radius):
    rng = np.random.default_rng(11)
    xs = [rng.integers(-2, 3, size=(n, 2)).astype(np.float32) for n in (150, 91, 40, 7)]
    ys = [rng.integers(-2, 3, size=(m, 2)).astype(np.float32) for m in (151, 130, 13, 7)]
    xs.append(np.repeat(np.arange(5, dtype=np.float32), 20)[:, None])           # long runs of equal frames: ties everywhere
    ys.append(np.repeat(np.arange(5, dtype=np.float32), 17)[:, None])
    _check_pairs(xs, ys, radius, exact_cost=True)


@pytest.mark.parametrize("radius", [1, 3])
def test_edge_lengths(radius):
    rng = np.random.default_rng(13)
    shapes = [(1, 1), (1, 7), (7, 1), (2, 2), (2, 3), (3, 3), (radius + 1, 50), (50, radius + 1), (radius + 2, radius + 2),
              (101, 99), (1100, 40), (40, 1100)]
    xs = [_walk(rng, n, 80) for n, _ in shapes]
    ys = [_walk(rng, m, 80) for _, m in shapes]
    _check_pairs(xs, ys, radius)


def _mse_batch(rng, B, dim=80):
    preds, targets, pl, tl = [], [], [], []
    for b in range(B):
        n, m = int(rng.integers(240, 1101)), int(rng.integers(240, 1001))
        a = _walk(rng, n, dim)
        c = _warp(rng, a, m)
        a[rng.random(n) < 0.1] = -4.0                   # unvoiced frames on both sides
        c[rng.random(m) < 0.1] = -4.0
        preds.append(a)
        targets.append(c)
        pl.append(n)
        tl.append(m)
    return _pad(preds), pl, _pad(targets), tl


def test_mse_after_dtw_matches_the_reference_and_none_for_unvoiced():
    from b2s_hip import metrics
    rng = np.random.default_rng(21)
    preds, pl, targets, tl = _mse_batch(rng, 6)
    preds[2] = -1.0                                      # an all-unvoiced prediction
    targets[4, :tl[4]] = -0.5                            # an all-unvoiced target
    got = metrics.calculate_mse_dtw(preds, pl, targets, tl)
    want = R.calculate_mse_dtw(preds, pl, targets, tl)
    for b, (g, w) in enumerate(zip(got, want)):
        if w is None:
            assert g is None, b
        else:
            assert isinstance(g, float) and abs(g - float(w)) <= 1e-5 * abs(float(w)), (b, g, w)
    assert got[2] is None and got[4] is None


def test_batch_independence_and_determinism():
    from b2s_hip import metrics
    rng = np.random.default_rng(31)
    preds, pl, targets, tl = _mse_batch(rng, 64)
    full = metrics.mse_dtw_batch(preds, pl, targets, tl).cpu().numpy()
    again = metrics.mse_dtw_batch(preds, pl, targets, tl).cpu().numpy()
    assert np.array_equal(full, again, equal_nan=True)
    alone = metrics.mse_dtw_batch(preds[17:18], pl[17:18], targets[17:18], tl[17:18]).cpu().numpy()
    assert alone[0] == full[17]
    c64, p64 = metrics.dtw_batch(preds, pl, targets, tl, radius=1, return_paths=True)
    c1, p1 = metrics.dtw_batch(preds[17:18], pl[17:18], targets[17:18], tl[17:18], radius=1, return_paths=True)
    assert float(c1[0]) == float(c64[17]) and np.array_equal(p1[0], p64[17])


def test_numpy_cpu_and_device_inputs_agree():
    from b2s_hip import metrics
    rng = np.random.default_rng(41)
    preds, pl, targets, tl = _mse_batch(rng, 3)
    a = metrics.calculate_mse_dtw(preds, pl, targets, tl)
    b = metrics.calculate_mse_dtw(torch.from_numpy(preds), torch.tensor(pl), torch.from_numpy(targets), np.array(tl))
    c = metrics.calculate_mse_dtw(torch.from_numpy(preds).cuda(), torch.tensor(pl).cuda(), torch.from_numpy(targets).cuda(),
                                  torch.tensor(tl).cuda())
    assert a == b == c
    d, path = metrics.fastdtw(preds[0, :pl[0]], targets[0, :tl[0]])
    rd, rpath = R.fastdtw(preds[0, :pl[0]], targets[0, :tl[0]])
    assert path == rpath and abs(d - rd) <= 1e-12 * rd


def test_eval_batch_with_mse_dtw_hip_feeds_the_reference_call(monkeypatch):
    """eval.py's sequence on the tiny model: eval_batch (which installs the metric for mse_dtw=hip), then
    infolog.calculate_mse_dtw(results['mel_aft'], results['generated_lengths'], <device targets>, <device lengths>)."""
    import sys
    import types
    import hyperparams
    import synthesize
    from hyperparams import hparams as hp
    from oracle import synth, make_config, TINY96
    from transformer.tacotron import Tacotron
    from b2s_hip import metrics
    infolog = types.ModuleType("utils.infolog")
    infolog.calculate_mse_dtw = R.calculate_mse_dtw
    monkeypatch.setitem(sys.modules, "utils.infolog", infolog)
    hp.override_from_dict(hyperparams.DEFAULTS)
    hp.parse(TINY96)
    hp.parse("compute_dtype=fp32,mse_dtw=hip,max_generation_frames=60")
    try:
        cfg = make_config(TINY96)
        st = synth.synthetic_state(cfg, 1234)
        m = Tacotron(hp)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in st.items()})
        m = m.to("cuda:0").eval()
        nb = synth.synthetic_batch(cfg, B=3, S=11, T=23, seed=7, in_lens=[11, 7, 4], tgt_lens=[23, 15, 9])
        batch = {k: (torch.from_numpy(np.asarray(v)).to("cuda:0") if not isinstance(v, list) else v) for k, v in nb.items()}
        results = synthesize.eval_batch(m, batch, use_bar=False, bar_interval=-1)
        assert infolog.calculate_mse_dtw is metrics.calculate_mse_dtw
        got = infolog.calculate_mse_dtw(results['mel_aft'], results['generated_lengths'], batch['mel_targets'], batch['target_lengths'])
        want = R.calculate_mse_dtw(np.asarray(results['mel_aft']), list(results['generated_lengths']),
                                   batch['mel_targets'].cpu().numpy(), batch['target_lengths'].cpu().numpy())
        assert len(got) == 3
        for g, w in zip(got, want):
            assert (g is None) == (w is None)
            if w is not None:
                assert abs(g - float(w)) <= 1e-5 * max(abs(float(w)), 1e-30), (g, w)
    finally:
        hp.override_from_dict(hyperparams.DEFAULTS)
        metrics.install(hp)
