"""GPU tests of MCD-DTW (b2s_hip.mcd, libb2s_mcd.so) against the NumPy restatement tests/mcd_ref.py.

One batch of 7 pairs with lengths {1, 2, 63, 64, 65, 129, 257} (the cepstral kernels cut utterances into chunks of 64 frames) and a
permutation of them on the other side; unvoiced frames at the start, in the middle, at the end, across the chunk boundaries, a frame
holding a NaN, one utterance with no voiced frame; mel values beyond +-4.  Gates: the fp32 cepstra, offsets, counts and paths are
EQUAL to the oracle's; the per-step distortion and the MCD are within 1e-12 relative (a step sums `order` squares, the mean at most
513 terms: the fp64 bound is under (513 + 260) * 2^-53 = 9e-14, and 1e-12 is the gate the DTW cost already has)."""
import json
import types
import zipfile

import numpy as np
import pytest
import torch

import mcd_ref as R

pytestmark = pytest.mark.gpu

LX = [1, 2, 63, 64, 65, 129, 257]
LY = [65, 129, 257, 65, 2, 1, 63]            # pair 3 is 64 x 65; the exact dtw of the batch stays under 40k cells
EMPTY_PAIR = 1                                # x side of pair 1 (2 frames) has no voiced frame
RTOL = 1e-12

# n_mels, order, symmetric_mel, radius
CONFIGS = [(80, 13, True, 1), (80, 13, True, None), (80, 79, False, 1), (80, 1, True, 1), (20, 13, False, None),
           (20, 19, True, 1), (20, 1, False, 1)]


def hp_of(symmetric):
    return types.SimpleNamespace(max_abs_value=4.0, max_db=100, ref_db=20, symmetric_mel=symmetric, data_format="nlti")


def walk(rng, T, n_mels, lim=5.0):
    return np.clip(np.cumsum(rng.standard_normal((T, n_mels)) * 0.3, axis=0), -lim, lim).astype(np.float32)


def make_batch(n_mels, symmetric):
    """Padded preds / targets of the 7 pairs.  With symmetric mels the walk reaches +-5, past the +-4 the scale clips at; without,
    it is shifted so that it covers [0, 1] and beyond."""
    rng = np.random.default_rng(20250301 + n_mels)
    xs = [walk(rng, n, n_mels) for n in LX]
    ys = [walk(rng, n, n_mels) for n in LY]
    if not symmetric:
        xs, ys = [x / 4 + 0.4 for x in xs], [y / 4 + 0.4 for y in ys]
    dead = np.float32(-4.0)
    xs[EMPTY_PAIR][:] = dead                              # no voiced frame at all
    xs[4][63:65] = dead                                   # across the chunk boundary, and the end
    xs[5][0:3] = dead                                     # the start
    xs[5][60:70] = dead                                   # across the first chunk boundary
    xs[6][0] = dead
    xs[6][100:111] = dead                                 # the middle
    xs[6][126:131] = dead                                 # across the second chunk boundary
    xs[6][250:257] = dead                                 # the end, into the last chunk of one frame
    xs[6][200, 7] = np.nan                                # a frame holding a NaN is dropped
    ys[1][63:65] = dead
    ys[1][128] = dead
    ys[2][191:194] = dead
    ys[2][40, 0] = np.nan
    ys[3][64] = 0.0                                       # a maximum of exactly 0 is not voiced
    preds = np.zeros((7, max(LX), n_mels), np.float32)
    targets = np.zeros((7, max(LY), n_mels), np.float32)
    for b in range(7):
        preds[b, :LX[b]] = xs[b]
        targets[b, :LY[b]] = ys[b]
    return preds, targets


_cache = {}


def case(cfg):
    """The batch, its oracle (computed once per configuration and left unchanged) and the GPU's details."""
    if cfg not in _cache:
        from b2s_hip import mcd
        n_mels, order, symmetric, radius = cfg
        hp = hp_of(symmetric)
        preds, targets = make_batch(n_mels, symmetric)
        ref = [R.mcd_dtw(preds[b, :LX[b]], targets[b, :LY[b]], order, radius, hp) for b in range(7)]
        out = mcd.mcd_dtw_details(preds, LX, targets, LY, order=order, radius=radius, hp=hp)
        host = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
        _cache[cfg] = (preds, targets, hp, ref, host)
    return _cache[cfg]


def ids(cfg):
    return "mels%d-order%d-%s-%s" % (cfg[0], cfg[1], "sym" if cfg[2] else "asym", "exact" if cfg[3] is None else "r%d" % cfg[3])


@pytest.mark.parametrize("cfg", CONFIGS, ids=ids)
def test_cepstra_offsets_and_counts_equal_the_oracle(cfg):
    preds, targets, hp, ref, got = case(cfg)
    for side, key in (("x", "cx"), ("y", "cy")):
        want = np.concatenate([r[key] for r in ref])
        counts = [len(r[key]) for r in ref]
        assert got["voiced_" + side].tolist() == counts
        assert got["offsets_" + side].tolist() == [0] + np.cumsum(counts).tolist()
        cep = got["cep_" + side]
        assert cep.shape == want.shape and cep.dtype == np.float32
        assert np.array_equal(cep.view(np.int32), want.view(np.int32)), \
            "%d of %d fp32 values differ, max |d| = %g" % ((cep != want).sum(), cep.size, np.abs(cep - want).max())
    assert got["voiced_x"][EMPTY_PAIR] == 0 and got["voiced_x"][6] == 257 - 1 - 11 - 5 - 7 - 1


@pytest.mark.parametrize("cfg", CONFIGS, ids=ids)
def test_paths_distortions_and_mcd(cfg):
    from b2s_hip import mcd
    preds, targets, hp, ref, got = case(cfg)
    po = got["path_offsets"]
    for b in range(7):
        if b == EMPTY_PAIR:
            assert ref[b]["mcd"] is None
            assert got["status"][b] == mcd.EMPTY and np.isnan(got["mcd"][b]) and got["path_len"][b] == 0
            continue
        n = int(got["path_len"][b])
        assert got["status"][b] == mcd.OK
        assert got["path"][po[b]:po[b] + n].tolist() == [list(p) for p in ref[b]["path"]]
        d, want = got["dist"][po[b]:po[b] + n], ref[b]["dist"]
        print("pair %d: max rel dist err %.3e, mcd %.12f vs %.12f" % (b, (np.abs(d - want) / want).max(), got["mcd"][b],
                                                                     ref[b]["mcd"]))
        assert want.min() > 0 and np.all(np.abs(d - want) <= RTOL * want)
        assert abs(got["mcd"][b] - ref[b]["mcd"]) <= RTOL * ref[b]["mcd"]


def test_list_function_and_the_empty_pair_leave_the_neighbours_alone():
    from b2s_hip import mcd
    cfg = CONFIGS[0]
    preds, targets, hp, ref, got = case(cfg)
    res = mcd.calculate_mcd_dtw(preds, LX, targets, LY, order=cfg[1], radius=cfg[3], hp=hp)
    assert res[EMPTY_PAIR] is None and all(type(v) is float for i, v in enumerate(res) if i != EMPTY_PAIR)
    assert [v for v in res if v is not None] == [float(v) for i, v in enumerate(got["mcd"]) if i != EMPTY_PAIR]
    keep = [b for b in range(7) if b != EMPTY_PAIR]
    without = mcd.mcd_dtw_batch(preds[keep], [LX[b] for b in keep], targets[keep], [LY[b] for b in keep], order=cfg[1], hp=hp)
    assert np.array_equal(without.cpu().numpy().view(np.int64), got["mcd"][keep].view(np.int64))
    assert mcd.calculate_mcd_dtw(preds[:0], [], targets[:0], []) == []


@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[4]], ids=ids)
def test_bits_repeat_and_do_not_depend_on_the_batch(cfg):
    from b2s_hip import mcd
    preds, targets, hp, ref, got = case(cfg)
    n_mels, order, symmetric, radius = cfg
    again = mcd.mcd_dtw_details(preds, LX, targets, LY, order=order, radius=radius, hp=hp)
    for key in ("mcd", "dist", "cep_x", "cep_y", "path_len"):
        a = again[key].cpu().numpy()
        assert np.array_equal(a.view(np.uint8), got[key].view(np.uint8)), key
    path, po = again["path"].cpu().numpy(), got["path_offsets"]
    for b in range(7):                                       # the rest of a pair's slot is not written
        n = int(got["path_len"][b])
        assert np.array_equal(path[po[b]:po[b] + n], got["path"][po[b]:po[b] + n])
    alone, paths = mcd.mcd_dtw_batch(preds[3:4], LX[3:4], targets[3:4], LY[3:4], order=order, radius=radius, hp=hp, return_paths=True)
    assert alone.shape == (1,) and alone.dtype == torch.float64                                    # B = 1
    assert alone.cpu().numpy().view(np.int64)[0] == got["mcd"].view(np.int64)[3]
    assert paths[0].tolist() == [list(p) for p in ref[3]["path"]]


def test_identity_is_exactly_zero():
    from b2s_hip import mcd
    preds, targets, hp, ref, got = case(CONFIGS[0])
    for radius in (1, None):
        m = mcd.mcd_dtw_batch(preds, LX, preds, LX, radius=radius, hp=hp).cpu().numpy()
        keep = [b for b in range(7) if b != EMPTY_PAIR]
        assert np.isnan(m[EMPTY_PAIR]) and np.all(m[keep] == 0.0), m


def test_a_uniform_gain_moves_only_c0():
    """x + 0.5 in every bin of an unclipped utterance shifts every log-magnitude by the same amount, which only c_0 sees: the
    cepstra differ by their fp32 rounding alone.  One fp32 ulp at |c| <= 64 is 7.6e-6 per coefficient, so the MCD stays under
    db_scale * sqrt(2 * 13) * 7.6e-6 = 1.7e-4 dB; the bound is 2e-4."""
    from b2s_hip import mcd
    rng = np.random.default_rng(77)
    x = np.round(walk(rng, 150, 80, lim=3.0) * 1024) / 1024          # on a grid, so that x + 0.5 is exact in fp32
    x = x.astype(np.float32)
    y = x + np.float32(0.5)
    assert np.all(x.max(axis=1) > 0) and np.abs(x).max() <= 3.0 and np.array_equal(y.astype(np.float64), x.astype(np.float64) + 0.5)
    hp = hp_of(True)
    got = float(mcd.mcd_dtw_batch(x[None], [150], y[None], [150], hp=hp)[0])
    want = R.mcd_dtw(x, y, hp=hp)["mcd"]
    print("uniform gain: gpu %.3e dB, oracle %.3e dB" % (got, want))
    assert 0.0 <= got <= 2e-4 and want <= 2e-4


def test_device_tensors_and_host_arrays_give_equal_results():
    from b2s_hip import mcd
    cfg = CONFIGS[0]
    preds, targets, hp, ref, got = case(cfg)
    dev = mcd.mcd_dtw_batch(torch.from_numpy(preds).cuda(), torch.tensor(LX).cuda(), torch.from_numpy(targets).cuda(),
                            torch.tensor(LY), order=cfg[1], radius=cfg[3], hp=hp)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy().view(np.int64), got["mcd"].view(np.int64))
    mixed = mcd.mcd_dtw_batch(torch.from_numpy(preds), np.asarray(LX), targets, LY, order=cfg[1], radius=cfg[3], hp=hp)
    assert np.array_equal(mixed.cpu().numpy().view(np.int64), got["mcd"].view(np.int64))
    cep, off, voiced = mcd.cepstra_batch(torch.from_numpy(preds).cuda(), LX, order=cfg[1], hp=hp)
    assert np.array_equal(cep.cpu().numpy(), got["cep_x"]) and off.cpu().tolist() == got["offsets_x"].tolist()
    assert voiced.cpu().tolist() == got["voiced_x"].tolist()


def test_inconsistent_offsets_fail_that_utterance_only(monkeypatch):
    from b2s_hip import mcd
    cfg = CONFIGS[0]
    preds, targets, hp, ref, got = case(cfg)
    t = torch.from_numpy(preds).cuda()
    pack = mcd.ragged.pack
    rows, off = pack(t, LX)
    bad = off.copy()
    bad[-1] += 3                                             # the last utterance runs 3 rows past the buffer
    out = mcd.cepstra_packed(rows, torch.from_numpy(bad).cuda(), max(LX) + 3, cfg[1], hp)
    status, voiced, offs = out["status"].cpu().numpy(), out["voiced"].cpu().numpy(), out["offsets"].cpu().numpy()
    assert status.tolist() == [mcd.OK, mcd.EMPTY, mcd.OK, mcd.OK, mcd.OK, mcd.OK, mcd.FAILED]
    assert voiced.tolist() == got["voiced_x"][:6].tolist() + [0] and offs.tolist() == got["offsets_x"][:7].tolist() + [offs[6]]
    n = int(offs[6])
    assert np.array_equal(out["cep"][:n].cpu().numpy(), got["cep_x"][:n])
    # decreasing (and the next utterance starts inside rows that utterance 1 claimed); negative; longer than max_len
    for wrong, failed in (([0, 1, 3, 2, 130, 195, 324, 581], [2, 3]), ([0, -1, 3, 66, 130, 195, 324, 581], [0, 1]),
                          ([0, 1, 3, 66, 130, 195, 195, 581], [6])):
        st = mcd.cepstra_packed(rows, torch.tensor(wrong, dtype=torch.int32).cuda(), max(LX), cfg[1], hp)["status"].cpu().tolist()
        assert [b for b, s in enumerate(st) if s == mcd.FAILED] == failed

    def bad_pack(t, lengths):
        rows, off = pack(t, lengths)
        off = off.copy()
        off[-1] += 3
        return rows, off
    monkeypatch.setattr(mcd.ragged, "pack", bad_pack)
    with pytest.raises(mcd.B2SError, match=r"failed for utterances \[6\]"):
        mcd.mcd_dtw_batch(preds, LX, targets, LY, hp=hp)
    res = mcd.mcd_dtw_details(preds, LX, targets, LY, hp=hp)
    assert res["status"].cpu().tolist() == [mcd.OK, mcd.EMPTY, mcd.OK, mcd.OK, mcd.OK, mcd.OK, mcd.FAILED]
    m = res["mcd"].cpu().numpy()
    assert np.array_equal(m[:6].view(np.int64), got["mcd"][:6].view(np.int64)) and np.isnan(m[6])


def test_overlapping_offsets_cannot_fill_more_rows_than_the_buffer_holds():
    """Offsets like [0, T, 0, T] are pairwise well formed after the decreasing utterance, but would compact 2 T voiced rows into a
    buffer of T: an utterance that starts inside rows an earlier one claimed is FAILED and writes nothing.  The call goes through
    the C ABI with guard rows behind the `total` rows the contract asks for; they must stay untouched."""
    from b2s_hip import mcd
    l = mcd.load()
    dev = torch.device("cuda")
    hp = hp_of(True)
    T, n_mels, order, guard = 300, 80, 13, 64
    x = walk(np.random.default_rng(9), T, n_mels, lim=4.0)
    want, keep = R.cepstra(x, order, hp)
    assert len(keep) == T
    rows = torch.from_numpy(x).to(dev)
    table = torch.from_numpy(mcd.dct_table(n_mels, order)).to(dev)

    def run(offsets, max_len):
        B = len(offsets) - 1
        off = torch.tensor(offsets, dtype=torch.int32, device=dev)
        cep = torch.full((T + guard, order), 12345.0, dtype=torch.float32, device=dev)
        out_off = torch.full((B + 1,), -7, dtype=torch.int32, device=dev)
        voiced = torch.full((B,), -7, dtype=torch.int32, device=dev)
        status = torch.full((B,), -7, dtype=torch.int32, device=dev)
        nbytes = l.b2s_mcd_ws_bytes(B, max_len)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        mcd.check(l.b2s_mcd_cepstra(rows.data_ptr(), off.data_ptr(), T, max_len, B, n_mels, order, table.data_ptr(), 1, 4.0, 100.0,
                                    20.0, R.LN_SCALE, cep.data_ptr(), out_off.data_ptr(), voiced.data_ptr(), status.data_ptr(),
                                    ws.data_ptr(), nbytes, None))
        torch.cuda.synchronize()
        return cep.cpu().numpy(), out_off.cpu().tolist(), voiced.cpu().tolist(), status.cpu().tolist()

    for offsets, st in (([0, T, 0, T], [mcd.OK, mcd.FAILED, mcd.FAILED]),
                        ([0, T, T // 2, T], [mcd.OK, mcd.FAILED, mcd.FAILED]),
                        ([0, 200, 100, T], [mcd.OK, mcd.FAILED, mcd.FAILED])):
        cep, out_off, voiced, status = run(offsets, T)
        n = offsets[1]
        assert status == st and voiced == [n, 0, 0] and out_off == [0, n, n, n]
        assert np.array_equal(cep[:n], want[:n]) and np.all(cep[n:] == 12345.0)
    # 300 utterances of one frame, so that the scan takes two rounds of 256: utterance 256 decreases, utterance 257 then starts
    # at row 3, inside what the FIRST round claimed, and spans 255 rows; the rest carry on from its end
    offsets = list(range(T + 1))
    offsets[257] = 3
    cep, out_off, voiced, status = run(offsets, T)
    assert [b for b, s in enumerate(status) if s != mcd.OK] == [256, 257] and status[256] == status[257] == mcd.FAILED
    assert voiced == [1] * 256 + [0, 0] + [1] * 42 and out_off[-1] == 298 and out_off[:257] == list(range(257))
    assert np.array_equal(cep[:256], want[:256]) and np.array_equal(cep[256:298], want[258:])
    assert np.all(cep[298:] == 12345.0)


def test_an_empty_batch_and_misshapen_files(tmp_path):
    from b2s_hip import mcd
    hp = hp_of(True)
    x = np.zeros((0, 5, 80), np.float32)
    m = mcd.mcd_dtw_batch(x, [], x, [], hp=hp)
    assert m.shape == (0,) and m.dtype == torch.float64
    assert mcd.mcd_dtw_batch(x, [], x, [], hp=hp, return_paths=True)[1] == []
    with pytest.raises(mcd.B2SError, match="holds no utterance"):
        mcd.mcd_dtw_details(x, [], x, [], hp=hp)
    data, ev = tmp_path / "data", tmp_path / "ev"
    data.mkdir()
    ev.mkdir()
    with zipfile.ZipFile(data / "mels.zip", "w") as z:
        with z.open("a.npy", "w") as f:
            np.save(f, walk(np.random.default_rng(1), 30, 80, lim=4.0))
    np.save(ev / "a.npy", np.zeros((30, 40), np.float32))             # generated with another number of bins
    with pytest.raises(mcd.B2SError, match=r"generated a\.npy has shape \(30, 40\), expected \[frames, 80\]"):
        mcd.score_eval_dir(str(ev), str(data / "mels.zip"), hp=hp)


def test_a_path_index_outside_the_voiced_count_is_not_followed():
    from b2s_hip import mcd
    l = mcd.load()
    dev = torch.device("cuda")
    cx = torch.arange(3 * 2, dtype=torch.float32, device=dev).reshape(3, 2)
    cy = cx + 1
    off = torch.tensor([0, 1, 3], dtype=torch.int32, device=dev)                 # pair 0: 1 x 1, pair 1: 2 x 2
    po = torch.tensor([0, 1, 4], dtype=torch.int32, device=dev)
    plen = torch.tensor([1, 3], dtype=torch.int32, device=dev)
    dstat = torch.zeros(2, dtype=torch.int32, device=dev)
    mcd_out = torch.zeros(2, dtype=torch.float64, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)

    def score(path):
        p = torch.tensor(path, dtype=torch.int32, device=dev)
        dist = torch.zeros(4, dtype=torch.float64, device=dev)
        mcd.check(l.b2s_mcd_score(cx.data_ptr(), off.data_ptr(), 3, cy.data_ptr(), off.data_ptr(), 3, 2, 2, p.data_ptr(), po.data_ptr(),
                                  4, plen.data_ptr(), dstat.data_ptr(), R.DB_SCALE, mcd_out.data_ptr(), status.data_ptr(),
                                  dist.data_ptr(), None))
        torch.cuda.synchronize()
        return status.cpu().tolist(), mcd_out.cpu().numpy(), dist.cpu().numpy()
    one = R.DB_SCALE * np.sqrt(2.0 * 2.0)                                         # cy - cx = 1 in both coefficients
    st, m, d = score([[0, 0], [0, 0], [1, 0], [1, 1]])
    assert st == [mcd.OK, mcd.OK] and abs(m[0] - one) <= RTOL * one and abs(d[3] - one) <= RTOL * one
    for wrong in ([1, 2], [-1, 0], [2, 1]):
        st, m, d = score([[0, 0], [0, 0], wrong, [1, 1]])
        assert st == [mcd.OK, mcd.FAILED] and abs(m[0] - one) <= RTOL * one and np.isnan(m[1]) and np.isnan(d[2])


def test_command_line_rescoring_of_a_finished_eval(tmp_path, capsys):
    from b2s_hip import mcd
    import hyperparams
    hp = hyperparams.hparams
    hp.override_from_dict(hyperparams.DEFAULTS)
    rng = np.random.default_rng(5)
    names = ["spk1_%02d" % i for i in range(6)]
    langs = ["en-us", "de-de", "en-us", "de-de", "en-us", "en-us"]
    truth = [walk(rng, int(n), 80, lim=4.0) for n in (40, 55, 64, 70, 33, 20)]
    truth[5][:] = -4.0                                               # a target with no voiced frame: counted as empty
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
    (ev / "transcriptions.jsonl").write_text("{}\n")                 # other files of an eval directory are not looked at
    out = tmp_path / "mcd.json"
    assert mcd.main([str(ev), "--data-dir", str(data), "--batch", "4", "--json", str(out)]) == 0
    printed = json.loads(capsys.readouterr().out)
    res = json.load(open(out))
    assert (res["n_scored"], res["n_empty"], res["n_without_target"]) == (5, 1, 1) and res["without_target"] == ["spk9_99"]
    assert printed["n_scored"] == 5 and "records" not in printed and printed["mcd"] == res["mcd"]
    recs = {r["name"]: r for r in res["records"]}
    assert sorted(recs) == names
    for n, g, m, l in zip(names, gen, truth, langs):
        want = R.mcd_dtw(g, m, 13, 1, hp)
        r = recs[n]
        assert r["language"] == l and r["voiced_pred"] == len(want["cx"]) and r["voiced_target"] == len(want["cy"])
        assert r["path_len"] == len(want["path"])
        if want["mcd"] is None:
            assert r["mcd"] is None and n == names[5]
        else:
            assert abs(r["mcd"] - want["mcd"]) <= RTOL * want["mcd"]
    for l in ("en-us", "de-de"):
        mine = [recs[n]["mcd"] for n, ll in zip(names, langs) if ll == l and recs[n]["mcd"] is not None]
        assert res["languages"][l] == {"n": len(mine), "mcd": float(np.mean(mine))}
    assert res["mcd"] == float(np.mean([r["mcd"] for r in res["records"] if r["mcd"] is not None]))
    assert mcd.main([str(ev), "--data-dir", str(data), "--radius", "exact", "--order", "20"]) == 0
    assert json.loads(capsys.readouterr().out)["radius"] == "exact"
