"""CPU-only tests of the MCD-DTW feature's host side: the C ABI of libb2s_mcd.so (declared, exported, bound, kept apart from the other
three libraries; every host-side refusal without a GPU), the DCT table, and the NumPy restatement (tests/mcd_ref.py) on properties
known in closed form."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mcd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = ["b2s_mcd_cepstra", "b2s_mcd_last_error", "b2s_mcd_score", "b2s_mcd_version", "b2s_mcd_ws_bytes"]


def walk(T, n_mels, seed, lim=4.0):
    rng = np.random.default_rng(seed)
    return np.clip(np.cumsum(rng.standard_normal((T, n_mels)) * 0.3, axis=0), -lim, lim).astype(np.float32)


# --------------------------------------------------------------------------------------------------------------------- the C ABI

def test_header_exports_and_prototypes_are_the_same_five_names():
    from b2s_hip import mcd
    l = mcd.load()
    header = open(os.path.join(ROOT, "include", "b2s_mcd.h")).read()
    declared = sorted(set(re.findall(r"\b(b2s_mcd_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert declared == mcd.EXPORTS == sorted(mcd._PROTOS) == ENTRY_POINTS
    for name in ENTRY_POINTS:
        assert hasattr(l, name)
    assert l.b2s_mcd_version() >= 100


def test_the_other_libraries_do_not_grow():
    from b2s_hip import lib, metrics, vocoder
    for mod in (lib, vocoder, metrics):
        assert not [n for n in mod.EXPORTS if n.startswith("b2s_mcd")]
    assert len(metrics.EXPORTS) == 9


def test_readme_carries_the_entry_point_count():
    assert "`libb2s_mcd.so`, %d entry points" % len(ENTRY_POINTS) in open(os.path.join(ROOT, "README.md")).read()


def test_importing_the_module_leaves_the_hyperparameters_alone():
    import hyperparams
    before = dict(hyperparams.DEFAULTS)
    from b2s_hip import mcd  # noqa: F401
    assert hyperparams.DEFAULTS == before
    assert "mcd" not in hyperparams.DEFAULTS and "mcd_dtw" not in hyperparams.DEFAULTS


def test_host_side_refusals_come_back_as_messages_without_a_gpu():
    from b2s_hip import mcd
    l = mcd.load()

    def err():
        return l.b2s_mcd_last_error().decode()
    d = C.c_void_p(16)                   # never dereferenced: every call below fails its checks before a launch
    good = dict(mel=d, off=d, total=100, max_len=50, B=2, n_mels=80, order=13, dct=d, cep=d, cep_off=d, voiced=d, status=d, ws=d,
                ws_bytes=1 << 20)

    def cep(**over):
        v = dict(good, **over)
        return l.b2s_mcd_cepstra(v["mel"], v["off"], v["total"], v["max_len"], v["B"], v["n_mels"], v["order"], v["dct"], 1, 4.0,
                                 100.0, 20.0, R.LN_SCALE, v["cep"], v["cep_off"], v["voiced"], v["status"], v["ws"], v["ws_bytes"],
                                 None)
    for bad in (0, -1):
        assert cep(B=bad) != 0 and "B must be > 0 (got %d)" % bad in err()
        assert l.b2s_mcd_ws_bytes(bad, 50) == 0 and "B must be > 0" in err()
    assert l.b2s_mcd_ws_bytes(2, -1) == 0 and "max_len must be >= 0" in err()
    assert l.b2s_mcd_ws_bytes(2, 50) > 0
    assert l.b2s_mcd_ws_bytes(1 << 14, 4096) > 0                                  # 2^20 chunks: the documented cap of one call
    assert l.b2s_mcd_ws_bytes(1 << 14, 4097) == 0 and "exceed the 1048576 chunks of one call" in err()
    assert cep(B=1 << 20, max_len=65) != 0 and "split the batch" in err()
    for bad in (0, 80, 257):
        assert cep(order=bad) != 0 and "order must be in 1..79 for 80 mel bins (got %d)" % bad in err()
    assert cep(order=257, n_mels=512) != 0 and "order must be in 1..256 for 512 mel bins (got 257)" in err()
    assert cep(n_mels=513) != 0 and "n_mels must be in 2..512" in err()
    assert cep(total=-1) != 0 and "total must be >= 0" in err()
    assert cep(off=None) != 0 and "offsets or dct is NULL" in err()
    assert cep(dct=None) != 0 and "offsets or dct is NULL" in err()
    assert cep(mel=None) != 0 and "mel or cep_out is NULL" in err()
    assert cep(cep=None) != 0 and "mel or cep_out is NULL" in err()
    for name in ("cep_off", "voiced", "status"):
        assert cep(**{name: None}) != 0 and "cep_offsets_out, voiced_out or status_out is NULL" in err()
    assert cep(ws=None) != 0 and "workspace" in err()
    assert cep(ws_bytes=8) != 0 and "workspace of 8 bytes" in err()

    sgood = dict(cx=d, cxo=d, tcx=10, cy=d, cyo=d, tcy=10, B=2, order=13, path=d, po=d, tp=20, plen=d, dstat=d, mcd=d, status=d)

    def score(**over):
        v = dict(sgood, **over)
        return l.b2s_mcd_score(v["cx"], v["cxo"], v["tcx"], v["cy"], v["cyo"], v["tcy"], v["B"], v["order"], v["path"], v["po"],
                               v["tp"], v["plen"], v["dstat"], R.DB_SCALE, v["mcd"], v["status"], None, None)
    for bad in (0, -3):
        assert score(B=bad) != 0 and "B must be > 0 (got %d)" % bad in err()
    for bad in (0, 257):
        assert score(order=bad) != 0 and "order must be in 1..256 (got %d)" % bad in err()
    for name in ("tcx", "tcy", "tp"):
        assert score(**{name: -1}) != 0 and "totals must be >= 0" in err()
    for name in ("cxo", "cyo", "po", "plen", "dstat"):
        assert score(**{name: None}) != 0 and "is NULL" in err()
    for name in ("cx", "cy", "path"):
        assert score(**{name: None}) != 0 and "cx, cy or path is NULL" in err()
    for name in ("mcd", "status"):
        assert score(**{name: None}) != 0 and "mcd_out or status_out is NULL" in err()


def test_python_surface_refuses_bad_sizes_before_any_gpu_work():
    from b2s_hip import mcd
    for n_mels, order in ((80, 0), (80, 80), (512, 257), (1, 1), (513, 13)):
        with pytest.raises(mcd.B2SError):
            mcd.dct_table(n_mels, order)


def test_there_is_no_cpu_fallback(monkeypatch):
    import torch
    from b2s_hip import mcd
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    x = walk(5, 80, 1)[None]
    with pytest.raises(mcd.B2SError, match="runs on the GPU only"):
        mcd.mcd_dtw_batch(x, [5], x, [5])


def test_command_line_usage_errors_are_nonzero(tmp_path, capsys):
    import hyperparams
    from b2s_hip import mcd
    hyperparams.hparams.override_from_dict(hyperparams.DEFAULTS)
    assert mcd.main([str(tmp_path / "nowhere"), "--data-dir", str(tmp_path)]) == 2
    assert mcd.main([str(tmp_path), "--data-dir", str(tmp_path)]) == 2                  # no mels.zip there
    assert mcd.main([str(tmp_path), "--data-dir", str(tmp_path), "--radius", "0"]) == 2
    for order in ("0", "80", "-3"):                                                     # 80 mel bins: c_1..c_79 at most
        assert mcd.main([str(tmp_path), "--data-dir", str(tmp_path), "--order", order]) == 2
    assert "--order must be in 1..79" in capsys.readouterr().err
    assert mcd.main([str(tmp_path), "--data-dir", str(tmp_path), "--batch", "0"]) == 2
    with pytest.raises(SystemExit) as e:
        mcd.main([])
    assert e.value.code == 2
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------------------------ the table

@pytest.mark.parametrize("n_mels,order", [(80, 13), (80, 79), (20, 1), (20, 19)])
def test_dct_rows_are_orthonormal(n_mels, order):
    """The mel sizes in use, up to the full order.  (The pinned formula rounds the cosine's argument, up to pi * order, to fp64, so
    the error of the table grows with order: 1e-14 is the bound at these sizes, not at 512 bins x 256 rows.)"""
    from b2s_hip import mcd
    D = mcd.dct_table(n_mels, order)
    assert D.shape == (order, n_mels) and D.dtype == np.float64
    assert np.abs(D @ D.T - np.eye(order)).max() <= 1e-14
    assert np.array_equal(D, R.dct_table(n_mels, order))
    assert np.abs(D.sum(axis=1)).max() <= 1e-13                 # every row is orthogonal to the constant: a gain moves c_0 only


def test_dct_rows_equal_scipy_when_it_is_there():
    fftpack = pytest.importorskip("scipy.fftpack")
    from b2s_hip import mcd
    for n_mels, order in ((80, 13), (20, 19)):
        full = fftpack.dct(np.eye(n_mels), type=2, norm="ortho", axis=0)           # column m = the transform of unit vector e_m
        assert np.abs(mcd.dct_table(n_mels, order) - full[1:order + 1]).max() <= 1e-14


# ----------------------------------------------------------------------------------------------------------------- the oracle

def test_loop_and_matrix_product_agree_in_every_fp32_value():
    x = walk(65, 80, 7, lim=5.0)
    c, keep = R.cepstra(x, 13)
    assert len(keep) == 65
    assert np.array_equal(c, (R.log_magnitude(x) @ R.dct_table(80, 13).T).astype(np.float32))


def test_oracle_identity_is_exactly_zero():
    x = walk(70, 80, 3)
    for radius in (1, None):
        assert R.mcd_dtw(x, x, radius=radius)["mcd"] == 0.0


def test_oracle_one_frame_pair_equals_the_closed_formula():
    x, y = walk(3, 80, 11)[2:], walk(4, 80, 12)[3:]
    assert x.shape == y.shape == (1, 80)
    D = R.dct_table(80, 13)
    cx = (R.log_magnitude(x[0]) @ D.T).astype(np.float32).astype(np.float64)
    cy = (R.log_magnitude(y[0]) @ D.T).astype(np.float32).astype(np.float64)
    want = 10.0 / np.log(10.0) * np.sqrt(2.0 * np.sum((cx - cy) ** 2))
    got = R.mcd_dtw(x, y)
    assert got["path"] == [(0, 0)] and want > 0
    assert abs(got["mcd"] - want) <= 1e-12 * want


def test_oracle_voiced_rule_and_the_empty_side():
    x = walk(9, 20, 5)
    x[2] = -4.0
    x[5, 3] = np.nan
    x[8] = 0.0                                                   # a maximum of exactly 0 is not voiced
    assert R.voiced(x).tolist() == [0, 1, 3, 4, 6, 7]
    assert R.mcd_dtw(np.full((4, 20), -4.0, np.float32), x)["mcd"] is None
    assert R.calculate_mcd_dtw([x, x[2:3]], [9, 1], [x, x], [9, 9], order=5) == [0.0, None]
