"""CPU-only tests of the duration feature's host side: the C ABI of libb2s_dur.so (declared, exported, bound, kept apart from the
other libraries; every host-side refusal without a GPU), the command line's usage errors, code_point_groups, scores_from_counts in
closed form, and the NumPy restatement (tests/dur_ref.py) on properties known in closed form."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import dur_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = ["b2s_dur_last_error", "b2s_dur_mas", "b2s_dur_score", "b2s_dur_version", "b2s_dur_ws_bytes"]


# --------------------------------------------------------------------------------------------------------------------- the C ABI

def test_header_exports_and_prototypes_are_the_same_five_names():
    from b2s_hip import durations
    l = durations.load()
    header = open(os.path.join(ROOT, "include", "b2s_dur.h")).read()
    declared = sorted(set(re.findall(r"\b(b2s_dur_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert declared == durations.EXPORTS == sorted(durations._PROTOS) == ENTRY_POINTS
    for name in ENTRY_POINTS:
        assert hasattr(l, name)
    assert l.b2s_dur_version() >= 100
    assert (durations.OK, durations.EMPTY, durations.FAILED, durations.SHORT) == (R.OK, R.EMPTY, R.FAILED, R.SHORT) == (0, 1, 2, 3)
    for name, value in (("OK", 0), ("EMPTY", 1), ("FAILED", 2), ("SHORT", 3), ("MAX_S", 1024), ("COUNTS", 12)):
        assert re.search(r"#define B2S_DUR_%s %d\b" % (name, value), header)
    assert durations.MAX_S == 1024 and len(durations.COUNTS) == R.N_COUNTS == 12


def test_the_other_libraries_do_not_grow():
    from b2s_hip import f0, lib, mcd, metrics, vocoder
    for mod in (lib, vocoder, metrics, mcd, f0):
        assert not [n for n in mod.EXPORTS if n.startswith("b2s_dur")]
    assert (len(vocoder.EXPORTS), len(metrics.EXPORTS), len(mcd.EXPORTS), len(f0.EXPORTS)) == (13, 9, 5, 5)


def test_readme_carries_the_entry_point_count():
    assert "`libb2s_dur.so`, %d entry points" % len(ENTRY_POINTS) in open(os.path.join(ROOT, "README.md")).read()


def test_importing_the_module_leaves_the_hyperparameters_alone():
    import hyperparams
    before = dict(hyperparams.DEFAULTS)
    from b2s_hip import durations  # noqa: F401
    assert hyperparams.DEFAULTS == before
    assert not [k for k in hyperparams.DEFAULTS if k.startswith("dur") or k.startswith("mas")]


def test_host_side_refusals_come_back_as_messages_without_a_gpu():
    from b2s_hip import durations
    l = durations.load()

    def err():
        return l.b2s_dur_last_error().decode()
    d = C.c_void_p(16)                   # never dereferenced: every call below fails its checks before a launch

    assert l.b2s_dur_ws_bytes(64, 256, 1000) == 64 * 1000 * 4 * 8
    assert l.b2s_dur_ws_bytes(3, 64, 7) == 3 * 7 * 8 and l.b2s_dur_ws_bytes(3, 65, 7) == 3 * 7 * 2 * 8
    assert l.b2s_dur_ws_bytes(1, 1024, 1100) == 1100 * 16 * 8
    for bad in (0, -1):
        assert l.b2s_dur_ws_bytes(bad, 256, 1000) == 0 and "B must be > 0 (got %d)" % bad in err()
    for bad in (0, -3, 1025):
        assert l.b2s_dur_ws_bytes(2, bad, 1000) == 0 and "S must be in 1..1024 (got %d)" % bad in err()
    for bad in (0, -1):
        assert l.b2s_dur_ws_bytes(2, 256, bad) == 0 and "T must be >= 1 (got %d)" % bad in err()
    assert l.b2s_dur_ws_bytes(1 << 30, 1024, 1 << 30) == 0 and "split the batch" in err()
    assert l.b2s_dur_ws_bytes(1 << 20, 1024, 1 << 11) == 0 and "split the batch" in err()      # 2^41 cells
    assert l.b2s_dur_ws_bytes(1 << 19, 1024, 1 << 11) == (1 << 30) * 16 * 8                     # 2^40 cells: the most one call takes

    good = dict(maps=d, enc=d, dec=d, B=2, S=256, T=1000, path=d, dur=d, score=d, status=d, ws=d, nbytes=2 * 1000 * 4 * 8)

    def mas(**over):
        v = dict(good, **over)
        return l.b2s_dur_mas(v["maps"], v["enc"], v["dec"], v["B"], v["S"], v["T"], v["path"], v["dur"], v["score"], v["status"],
                             v["ws"], v["nbytes"], None)
    for bad in (0, -2):
        assert mas(B=bad) != 0 and "B must be > 0 (got %d)" % bad in err()
    for bad in (0, 1025, -1):
        assert mas(S=bad) != 0 and "S must be in 1..1024 (got %d)" % bad in err()
    assert mas(T=0) != 0 and "T must be >= 1 (got 0)" in err()
    assert mas(B=1 << 30, T=1 << 30) != 0 and "split the batch" in err()
    for name in ("maps", "enc", "dec"):
        assert mas(**{name: None}) != 0 and "maps, enc_len or dec_len is NULL" in err()
    for name in ("path", "dur", "score", "status"):
        assert mas(**{name: None}) != 0 and "path, durations, score or status is NULL" in err()
    assert mas(nbytes=good["nbytes"] - 1) != 0 and "workspace of 63999 bytes, 64000 needed" in err()
    assert mas(ws=None) != 0 and "workspace of 0 bytes, 64000 needed" in err()
    assert mas(ws=C.c_void_p(20)) != 0 and "8-byte aligned" in err()

    sgood = dict(x=d, y=d, enc=d, groups=None, B=2, S=256, counts=d, status=d)

    def score(**over):
        v = dict(sgood, **over)
        return l.b2s_dur_score(v["x"], v["y"], v["enc"], v["groups"], v["B"], v["S"], v["counts"], v["status"], None)
    for bad in (0, -7):
        assert score(B=bad) != 0 and "B must be > 0 (got %d)" % bad in err()
    for bad in (0, 1025):
        assert score(S=bad) != 0 and "S must be in 1..1024 (got %d)" % bad in err()
    for name in ("x", "y", "enc"):
        assert score(**{name: None}) != 0 and "dur_x, dur_y or enc_len is NULL" in err()
    for name in ("counts", "status"):
        assert score(**{name: None}) != 0 and "counts or status is NULL" in err()


def test_there_is_no_cpu_fallback(monkeypatch):
    import torch
    from b2s_hip import durations
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    maps = np.ones((1, 3, 5), np.float32)
    with pytest.raises(durations.B2SError, match="runs on the GPU only"):
        durations.mas_batch(maps, [3], [5])
    with pytest.raises(durations.B2SError, match="runs on the GPU only"):
        durations.byte_durations([maps[:, None]], [3], [5])
    with pytest.raises(durations.B2SError, match="runs on the GPU only"):
        durations.duration_error_batch(np.ones((1, 3), np.int32), np.ones((1, 3), np.int32), [3])
    with pytest.raises(durations.B2SError, match="runs on the GPU only"):
        durations.teacher_forced_durations(torch.nn.Linear(2, 2), {})


def test_command_line_usage_errors_are_nonzero(tmp_path, capsys):
    import hyperparams
    from b2s_hip import durations
    hyperparams.hparams.override_from_dict(hyperparams.DEFAULTS)
    ckpt = tmp_path / "model.ckpt-1"
    ckpt.write_bytes(b"not read before the usage checks")
    out = str(tmp_path / "out")
    assert durations.main([str(tmp_path / "nowhere"), "--data-dir", str(tmp_path), "--out", out]) == 2     # no checkpoint
    assert "checkpoint not found" in capsys.readouterr().err
    assert durations.main([str(ckpt), "--data-dir", str(tmp_path), "--out", out]) == 2                     # no mels.zip there
    assert "mels.zip not found" in capsys.readouterr().err
    assert durations.main([str(ckpt), "--data-dir", str(tmp_path), "--out", out, "--batch", "0"]) == 2
    assert "--batch must be >= 1" in capsys.readouterr().err
    assert durations.main([str(ckpt), "--data-dir", str(tmp_path), "--out", out, "--units", "words"]) == 2
    assert "--units must be" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        durations.main([])
    assert e.value.code == 2
    capsys.readouterr()
    assert not os.path.exists(out)


# ----------------------------------------------------------------------------------------------------------------- code points

def test_code_point_groups_follow_utf8():
    from b2s_hip import durations
    from utils.text import text_to_byte_sequence
    texts = ["abc", "é", "a€b", "😀!", "模型 tts", ""]
    seqs = [text_to_byte_sequence(t) for t in texts]
    S = max(len(s) for s in seqs) + 2
    ids = np.zeros((len(seqs), S), np.int64)
    for i, s in enumerate(seqs):
        ids[i, :len(s)] = s
    n = [len(s) for s in seqs]
    got = durations.code_point_groups(ids, n).numpy()
    assert got.dtype == np.int32 and got.shape == ids.shape
    assert got[0, :5].tolist() == [0, 1, 2, 3, 4]                          # sos a b c eos
    assert got[1, :4].tolist() == [0, 1, 1, 2]                             # sos, two bytes of one character, eos
    assert got[2, :7].tolist() == [0, 1, 2, 2, 2, 3, 4]                    # three bytes
    assert got[3, :7].tolist() == [0, 1, 1, 1, 1, 2, 3]                    # four bytes
    assert got[5, :2].tolist() == [0, 1]                                   # sos eos alone
    for i, (t, s) in enumerate(zip(texts, seqs)):
        assert got[i, :n[i]].tolist() == R.code_point_groups(s, n[i])
        assert got[i, n[i] - 1] + 1 == len(t) + 2                          # one unit per code point, and sos and eos
        assert np.all(got[i, n[i]:] == -1)
    import torch
    assert torch.equal(durations.code_point_groups(torch.from_numpy(ids), torch.tensor(n)), torch.from_numpy(got))
    lone = durations.code_point_groups(np.array([[0x80, 0x80, 0x41]]), [3]).numpy()
    assert lone.tolist() == [[0, 0, 1]]                                    # a continuation byte in front still starts at 0


# ------------------------------------------------------------------------------------------------------------------ the scores

def test_scores_from_counts_in_closed_form():
    from b2s_hip import durations
    same = [3, 1, 4, 1, 5, 9, 2, 6]
    c, st = R.counts(same, same, len(same))
    assert st == R.OK and c[:3] == [8, 31, 31] and c[3] == 0 and c[4] == 0 and c[5] == c[6] == c[7] and c[8:] == [9, 9, 0, 0]
    s = durations.scores_from_counts(np.array([c], np.int64), 12.5)
    assert s["rmse_frames"][0] == 0.0 and s["rmse_ms"][0] == 0.0 and s["mae_frames"][0] == 0.0
    assert s["rate_ratio"][0] == 1.0 and s["pearson"][0] == 1.0

    c, st = R.counts([2, 2, 2, 2], [1, 2, 3, 4], 4)                        # a constant side has no correlation
    s = durations.scores_from_counts(np.array(c, np.int64), 10.0)
    assert st == R.OK and math.isnan(s["pearson"]) and s["rate_ratio"] == 0.8

    c, st = R.counts([1, 2, 3, 4], [2, 2, 2, 4], 4)                        # by hand: n 4, sums 10 / 10, |d| 2, d^2 2, 30, 28, 28
    assert st == R.OK and c == [4, 10, 10, 2, 2, 30, 28, 28, 4, 4, 0, 0]
    s = durations.scores_from_counts(np.array([c], np.int64), 12.5)
    assert s["rmse_frames"][0] == math.sqrt(0.5) and s["rmse_ms"][0] == math.sqrt(0.5) * 12.5 and s["mae_frames"][0] == 0.5
    assert s["rate_ratio"][0] == 1.0 and s["pearson"][0] == 12 / math.sqrt(20 * 12)

    s = durations.scores_from_counts(np.zeros((2, 12), np.int64), 12.5)    # EMPTY / FAILED rows
    assert all(np.isnan(s[k]).all() for k in durations.SCORES)
    with pytest.raises(durations.B2SError):
        durations.scores_from_counts(np.zeros((1, 12), np.int32), 12.5)


def test_oracle_counts_with_groups_and_refusals():
    x, y = [1, 2, 3, 4, 5, 0], [2, 2, 2, 4, 0, 5]
    c, st = R.counts(x, y, 5, groups=[0, 0, 1, 2, 2, 7])                   # units (3, 3, 9) and (4, 2, 4); position 5 is past n
    assert st == R.OK and c == [3, 15, 10, 7, 1 + 1 + 25, 9 + 9 + 81, 16 + 4 + 16, 12 + 6 + 36, 9, 4, 0, 0]
    c, st = R.counts(x, y, 5, groups=[0] * 6)                              # one unit over the whole utterance
    assert st == R.OK and c == [1, 15, 10, 5, 25, 225, 100, 150, 15, 10, 0, 0]
    c, st = R.counts(x, y, 6)
    assert st == R.OK and c[10:] == [1, 1]                                 # a position without a frame on either side
    assert R.counts(x, y, 0) == ([0] * 12, R.EMPTY)
    for bad in (dict(n=7), dict(n=-1), dict(n=5, groups=[1, 1, 2, 3, 4, 5]), dict(n=5, groups=[0, 2, 2, 3, 4, 5]),
                dict(n=5, groups=[0, 1, 0, 1, 2, 3])):
        assert R.counts(x, y, **bad) == ([0] * 12, R.FAILED)
    assert R.counts([1, -1], [1, 1], 2)[1] == R.FAILED
    assert R.counts([2 ** 31 - 1, 1], [1, 1], 2)[1] == R.FAILED and R.counts([2 ** 31 - 2, 1], [1, 1], 2)[1] == R.OK


# ------------------------------------------------------------------------------------------------------------------ the oracle

SHAPES = [(1, 1), (1, 9), (2, 2), (63, 200), (65, 257), (129, 515), (256, 1000)]


def test_a_uniform_map_leaves_every_tie_where_it_is():
    """All paths score the same, `move` is strict, so the walk back from the last position steps down as late as it can: every
    position but the last gets one frame."""
    for S, T in ((5, 12), (1, 4), (64, 64), (65, 300)):
        r = R.mas(np.full((S, T), 0.25, np.float32), S, T)
        assert r["status"] == R.OK and r["durations"].tolist() == [1] * (S - 1) + [T - S + 1] and r["score"] == 0.25 * T
    assert R.mas(np.ones((5, 12), np.float32), 5, 12)["durations"].tolist() == [1, 1, 1, 1, 8]


def test_equal_lengths_leave_one_path():
    rng = np.random.default_rng(1)
    for S in (1, 2, 7, 64, 200):
        p = rng.random((S, S)).astype(np.float32)
        r = R.mas(p, S, S)
        assert r["durations"].tolist() == [1] * S and r["path"].tolist() == list(range(S))
        assert r["score"] == float(np.cumsum(np.diag(p).astype(np.float64))[-1])       # the same adds in the same order


@pytest.mark.parametrize("S,T", SHAPES)
def test_a_planted_staircase_is_recovered(S, T):
    rng = np.random.default_rng(100 * S + T)
    d = R.random_durations(rng, S, T)
    assert d.min() >= 1 and d.sum() == T
    p = np.full((S + 3, T + 5), np.nan, np.float32)                        # the padding is never looked at
    p[:S, :T] = R.staircase(rng, d)
    r = R.mas(p, S, T)
    assert r["status"] == R.OK and r["durations"][:S].tolist() == d.tolist() and not r["durations"][S:].any()
    path = r["path"][:T]
    assert path[0] == 0 and path[-1] == S - 1 and set(np.diff(path).tolist()) <= {0, 1} and np.all(r["path"][T:] == -1)
    assert r["score"] == float(np.cumsum(p[path, np.arange(T)].astype(np.float64))[-1])


def test_the_path_is_monotonic_on_any_map_and_beats_random_paths():
    rng = np.random.default_rng(7)
    for S, T in ((3, 9), (17, 40), (70, 131)):
        p = rng.random((S, T)).astype(np.float32) ** 4
        r = R.mas(p, S, T)
        path = r["path"]
        assert path[0] == 0 and path[-1] == S - 1 and set(np.diff(path).tolist()) <= {0, 1}
        assert r["durations"].sum() == T and r["durations"].min() >= 1
        for _ in range(20):
            other = np.repeat(np.arange(S), R.random_durations(rng, S, T))
            assert float(p[other, np.arange(T)].astype(np.float64).sum()) <= r["score"] + 1e-9


def test_oracle_statuses():
    p = np.ones((4, 6), np.float32)
    assert R.mas(p, 0, 6)["status"] == R.EMPTY and R.mas(p, 4, 0)["status"] == R.EMPTY and R.mas(p, 0, 6)["score"] == 0.0
    assert R.mas(p, 4, 3)["status"] == R.SHORT and math.isnan(R.mas(p, 4, 3)["score"])
    for Sb, Tb in ((5, 6), (4, 7), (-1, 6)):
        assert R.mas(p, Sb, Tb)["status"] == R.FAILED
    q = p.copy()
    q[3, 5] = np.inf
    assert R.mas(q, 4, 6)["status"] == R.FAILED and R.mas(q, 3, 6)["status"] == R.OK and R.mas(q, 4, 5)["status"] == R.OK
    r = R.mas(q, 4, 6)
    assert np.all(r["path"] == -1) and not r["durations"].any() and math.isnan(r["score"])
