"""The GPU alignment-head selection (b2s_hip.alignment, b2s_met_align_select of libb2s_metrics.so) against the fp64 NumPy restatement
of its contract and the restated selection loop of the reference's plot_attn (tests/align_ref.py).

The choice, the paths and the statistics must be exact and the maps bit-equal to the source slab.  The scores are fp64 sums of at
most 1100 fp32 maxima in [0, 1] in two different (fixed) orders: n * 2^-53 * sum is about 1.3e-10, the gate is 1e-9 absolute.  Inputs
hold 7.0 past either length, so a single read past a length moves a score by far more than that."""
import json
import os

import numpy as np
import pytest
import torch

import align_ref as R

pytestmark = pytest.mark.gpu

_cache = {}


def _chunk():
    from b2s_hip import alignment
    return alignment.chunk()


def _case(name, tie=False):
    """(layers, enc, dec, restatement (a)) of one generator case, computed once and shared; never modified by the tests."""
    key = (name, tie)
    if key not in _cache:
        B, L, H, S, T, enc, dec = R.gpu_cases(_chunk())[name]
        layers = R.make_case(R.SEED, B, L, H, S, T, enc, dec)
        want = None
        if tie:
            want = R.duplicate_best(layers, R.select(layers, enc, dec)["best"])
        _cache[key] = (layers, enc, dec, R.select(layers, enc, dec), want)
    return _cache[key]


def _run(layers, enc, dec, **kw):
    from b2s_hip import alignment
    out = alignment.select_alignments([torch.from_numpy(a).cuda() for a in layers], enc, dec, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


CASES = ["ragged", "two_chunks_odd", "two_chunks_vec", "two_chunks_vec_deep", "sixteen_layers"]


@pytest.mark.parametrize("name", CASES)
def test_selection_matches_the_contract(name):
    layers, enc, dec, ref, _ = _case(name)
    H = layers[0].shape[1]
    got = _run(layers, enc, dec)
    err = np.abs(got["scores"] - ref["scores"]).max()
    print("%s: max |score - fp64 restatement| = %.3e" % (name, err))
    assert err <= 1e-9
    best = np.where(got["layer"] >= 0, got["layer"] * H + got["head"], -1)
    assert np.array_equal(best, ref["best"])
    assert np.array_equal(got["paths"], ref["paths"])
    assert np.array_equal(got["stats"], ref["stats"])
    assert got["maps"].dtype == np.float32 and np.array_equal(got["maps"].view(np.uint32), ref["maps"].view(np.uint32))
    for b in range(len(enc)):
        want = ref["scores"][b].reshape(-1)[ref["best"][b]] / max(min(dec[b], layers[0].shape[3]), 1) if ref["best"][b] >= 0 else 0.0
        assert abs(got["focus"][b] - want) <= 1e-9
    # bit-reproducible: fixed summation order, no floating-point atomics
    again = _run(layers, enc, dec)
    assert np.array_equal(got["scores"].view(np.uint64), again["scores"].view(np.uint64))


def test_zero_dec_len_gives_no_choice():
    layers, enc, dec, ref, _ = _case("ragged")
    assert dec[3] == 0
    got = _run(layers, enc, dec)
    assert got["layer"][3] == -1 and got["head"][3] == -1 and got["focus"][3] == 0.0
    assert not got["maps"][3].any() and (got["paths"][3] == -1).all() and not got["stats"][3].any() and not got["scores"][3].any()
    got = _run(layers, [0, 0, 0, 0], dec)               # enc_len 0 is the same state
    assert (got["layer"] == -1).all() and not got["maps"].any() and (got["paths"] == -1).all() and not got["stats"].any()


def test_null_outputs_leave_scores_and_choice_unchanged():
    import ctypes as C
    from b2s_hip import metrics
    layers, enc, dec, ref, _ = _case("ragged")
    B, H, S, T = layers[0].shape
    L = len(layers)
    lib = metrics.load()
    dev = [torch.from_numpy(a).cuda() for a in layers]
    enc_d, dec_d = torch.tensor(enc, dtype=torch.int32).cuda(), torch.tensor(dec, dtype=torch.int32).cuda()
    nbytes = lib.b2s_met_align_ws_bytes(B, L, H, S, T)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    scores = torch.empty(B, L, H, dtype=torch.float64, device="cuda")
    best = torch.empty(B, dtype=torch.int32, device="cuda")
    table = (C.c_void_p * L)(*[t.data_ptr() for t in dev])
    metrics.check(lib.b2s_met_align_select(table, L, B, H, S, T, enc_d.data_ptr(), dec_d.data_ptr(), scores.data_ptr(), best.data_ptr(),
                                           None, None, None, ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream))
    full = _run(layers, enc, dec)
    assert np.array_equal(scores.cpu().numpy().view(np.uint64), full["scores"].view(np.uint64))
    assert np.array_equal(best.cpu().numpy(), ref["best"])
    assert "maps" not in _run(layers, enc, dec, want_maps=False)


@pytest.mark.parametrize("name", CASES)
def test_choice_agrees_with_the_reference_fp32_loop(name):
    """The reference's running fp32 sum errs by at most T * 2^-24 * score <= 7e-5 * T: where the best two fp64 scores are at least
    1e-3 * dec_len apart (asserted on these very inputs, no utterance excepted) both rules must name the same head."""
    layers, enc, dec, ref, _ = _case(name)
    H = layers[0].shape[1]
    got = _run(layers, enc, dec)
    for b in range(len(enc)):
        if dec[b] > 0:
            assert R.best_gap(ref["scores"][b]) >= 1e-3 * dec[b], (name, b)
        k, h, _crop = R.plot_attn_choice([a[b].transpose(0, 2, 1) for a in layers], enc[b], dec[b])
        if dec[b] > 0:
            assert (got["layer"][b], got["head"][b]) == (k, h), (name, b)


def test_exact_tie_picks_the_earlier_head_under_both_rules():
    layers, enc, dec, ref, want = _case("ragged", tie=True)
    H = layers[0].shape[1]
    assert np.array_equal(ref["best"], want)
    got = _run(layers, enc, dec)
    assert np.array_equal(np.where(got["layer"] >= 0, got["layer"] * H + got["head"], -1), want)
    for b in range(len(enc)):
        if dec[b] > 0:
            k, h, _crop = R.plot_attn_choice([a[b].transpose(0, 2, 1) for a in layers], enc[b], dec[b])
            assert k * H + h == want[b]
            s = np.sort(ref["scores"][b].reshape(-1))
            assert s[-1] == s[-2]                        # the tie is exact


def test_numpy_and_host_tensor_inputs_agree_with_device_inputs():
    from b2s_hip import alignment
    layers, enc, dec, ref, _ = _case("two_chunks_odd")
    a = _run(layers, enc, dec)
    b = {k: v.cpu().numpy() for k, v in alignment.select_alignments(layers, np.array(enc), torch.tensor(dec)).items()}
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_eval_batch_with_align_hip_returns_the_head_the_reference_would_plot(tmp_path):
    """eval.py's sequence on the tiny fp32 model, dropout off: align=reference and align=hip from the same decode seed."""
    import hyperparams
    import synthesize
    from hyperparams import hparams as hp
    from oracle import synth, make_config, TINY96
    from transformer.tacotron import Tacotron
    hp.override_from_dict(hyperparams.DEFAULTS)
    hp.parse(TINY96)
    hp.parse("compute_dtype=fp32,max_generation_frames=60")
    try:
        cfg = make_config(TINY96)
        st = synth.synthetic_state(cfg, 1234)
        m = Tacotron(hp)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in st.items()})
        m = m.to("cuda:0").eval()
        nb = synth.synthetic_batch(cfg, B=3, S=11, T=23, seed=7, in_lens=[11, 7, 4], tgt_lens=[23, 15, 9])
        batch = {k: (torch.from_numpy(np.asarray(v)).to("cuda:0") if not isinstance(v, list) else v) for k, v in nb.items()}
        batch["names"] = ["utt%d" % i for i in range(3)]
        ref = synthesize.eval_batch(m, batch, use_bar=False, bar_interval=-1)
        hp.parse("align=hip")
        res = synthesize.eval_batch(m, batch, use_bar=False, bar_interval=-1)
        dev = synthesize.eval_batch(m, batch, use_bar=False, bar_interval=-1, device_results=True)
        assert np.array_equal(res["mel_pre"], ref["mel_pre"]) and np.array_equal(res["mel_aft"], ref["mel_aft"])
        assert [int(n) for n in res["generated_lengths"]] == [int(n) for n in ref["generated_lengths"]]
        L, H = len(ref["alignments"]["encdec"]), ref["alignments"]["encdec"][0].shape[1]
        assert L > 1 or H > 1
        want = R.select(ref["alignments"]["encdec"], ref["input_lengths"], ref["generated_lengths"])
        sel = res["alignments"]["selected"]
        enc = res["alignments"]["encdec"]
        assert len(enc) == 1 and enc[0].shape == (3, 1) + ref["alignments"]["encdec"][0].shape[2:]
        assert sel["scores"].shape == (3, L, H) and sel["stats"].shape == (3, 4)
        for b in range(3):
            assert int(ref["generated_lengths"][b]) > 0
            assert R.best_gap(want["scores"][b]) > 1e-9, b
            assert int(sel["layer"][b]) * H + int(sel["head"][b]) == want["best"][b]
            src = ref["alignments"]["encdec"][int(sel["layer"][b])][b, int(sel["head"][b])]
            assert np.array_equal(enc[0][b, 0].view(np.uint32), src.view(np.uint32))
            assert np.array_equal(sel["stats"][b], want["stats"][b])
            # an unedited plot_attn over the one returned map draws the chosen head's crop of the reference mode
            n_in, n_out = int(ref["input_lengths"][b]), int(ref["generated_lengths"][b])
            k1, h1, crop1 = R.plot_attn_choice([a[b].transpose(0, 2, 1) for a in enc], n_in, n_out)
            assert (k1, h1) == (0, 0) and np.array_equal(crop1, src.T[:n_out, :n_in])
        assert np.abs(sel["scores"] - want["scores"]).max() <= 1e-9
        assert res["alignments"]["self"] == ref["alignments"]["self"] == []
        assert isinstance(sel["layer"], np.ndarray) and isinstance(enc[0], np.ndarray)
        # device_results=True: tensors on the device, the same values
        d_al = dev["alignments"]
        assert d_al["encdec"][0].is_cuda and all(v.is_cuda for v in d_al["selected"].values())
        assert np.array_equal(d_al["encdec"][0].cpu().numpy(), enc[0])
        assert np.array_equal(d_al["selected"]["layer"].cpu().numpy(), sel["layer"])
        synthesize.save_eval_results(**res, output_dir=str(tmp_path))
        for b, name in enumerate(batch["names"]):
            assert (tmp_path / ("%s.npy" % name)).exists()
            info = json.load(open(os.path.join(str(tmp_path), "%s_align.json" % name)))
            assert (info["layer"], info["head"]) == (int(sel["layer"][b]), int(sel["head"][b]))
            assert [info[k] for k in ("backward_steps", "max_jump", "positions_visited", "last_position")] == want["stats"][b].tolist()
    finally:
        hp.override_from_dict(hyperparams.DEFAULTS)
