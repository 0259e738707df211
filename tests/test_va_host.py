"""CPU-only tests of the variance adaptor's host side: the C ABI of libb2s_va.so (declared, exported, bound, kept apart from the
other libraries; every host-side refusal without a GPU) and the NumPy restatement (tests/va_ref.py) against independent ground on
inputs for which no order matters: with integers in -8..8 every fp32 sum is exact, so the restatement must EQUAL torch's CPU
autograd of (x + embedding(pb)) + embedding(eb) followed by repeat_interleave."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import va_ref as R
from test_pros_host import dynamic_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = ["b2s_va_backward", "b2s_va_forward", "b2s_va_frames", "b2s_va_last_error", "b2s_va_pad", "b2s_va_quantise",
                "b2s_va_version", "b2s_va_ws_bytes"]


# --------------------------------------------------------------------------------------------------------------------- the C ABI

def test_header_exports_and_prototypes_are_the_same_names():
    from b2s_hip import variance
    l = variance.load()
    header = open(os.path.join(ROOT, "include", "b2s_va.h")).read()
    declared = sorted(set(re.findall(r"\b(b2s_va_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))))
    assert declared == variance.EXPORTS == sorted(variance._PROTOS) == ENTRY_POINTS
    assert sorted(n for n in dynamic_symbols(variance.LIB_PATH) if n.startswith("b2s_")) == ENTRY_POINTS       # exactly these
    for name in ENTRY_POINTS:
        assert hasattr(l, name)
    assert l.b2s_va_version() >= 100
    assert (variance.OK, variance.EMPTY, variance.FAILED) == (R.OK, R.EMPTY, R.FAILED) == (0, 1, 2)
    assert variance.STATUS_NAMES == ("OK", "EMPTY", "FAILED")
    for name, value in (("OK", "0"), ("EMPTY", "1"), ("FAILED", "2"), ("MAX_S", "1024"), ("MAX_D", "1024"), ("MAX_BINS", "256"),
                        ("MAX_FRAMES", r"\(1 << 20\)")):
        assert re.search(r"#define B2S_VA_%s %s(\s|$)" % (name, value), header), name
    assert (variance.MAX_S, variance.MAX_D, variance.MAX_BINS, variance.MAX_FRAMES) == (1024, 1024, 256, 1 << 20)
    assert (R.MAX_S, R.MAX_D, R.MAX_BINS, R.MAX_FRAMES) == (1024, 1024, 256, 1 << 20)


def test_the_binding_follows_the_shared_loader():
    from b2s_hip import B2SError, cbind, durations, f0, lib, mcd, metrics, prosody, variance, vocoder
    assert variance.B2SError is cbind.B2SError is B2SError
    assert variance.LIB_PATH == variance._LIB.path and variance.LIB_PATH.endswith("few-shot-transformer-tts_amd/libb2s_va.so")
    assert variance.EXPORTS == variance._LIB.exports == sorted(variance._PROTOS) and variance._LIB.protos is variance._PROTOS
    assert variance.load() is variance.load()                              # cached
    assert variance.check(0) is None
    assert (variance.OK, variance.EMPTY, variance.FAILED) == (cbind.OK, cbind.EMPTY, cbind.FAILED)
    for mod in (lib, vocoder, metrics, mcd, f0, durations, prosody):       # the other libraries do not grow
        assert not [n for n in mod.EXPORTS if n.startswith("b2s_va")]
    protos = dict(variance._PROTOS, b2s_va_no_such_entry=(C.c_int, []))
    with pytest.raises(AttributeError, match="b2s_va_no_such_entry"):
        cbind.Library("libb2s_va.so", protos, "b2s_va_last_error").load()
    # an error slot of its own: a refusal here does not show up in, or overwrite, the prosody library's
    assert prosody.load().b2s_pros_ws_bytes(10, 0, 5) == 0
    assert variance.load().b2s_va_ws_bytes(2, 0, 8, 4) == 0
    with pytest.raises(B2SError, match=r"^S must be in 1..1024 \(got 0\)$"):
        variance.check(1)
    with pytest.raises(B2SError, match=r"^tau_min must be >= 1 \(got 0\)$"):
        prosody.check(1)
    with pytest.raises(B2SError, match=r"S must be in 1..1024 \(got 0\)"):
        variance.workspace(0, "cpu")                                       # 0 bytes is the library's refusal
    ws = variance.workspace(variance.load().b2s_va_ws_bytes(3, 5, 8, 2), "cpu")
    assert ws.dtype == torch.uint8 and ws.numel() == 16 + 2 * (512 + 256)


def test_readme_carries_the_entry_point_count():
    assert len(ENTRY_POINTS) == 8
    assert "`libb2s_va.so`, 8 entry points" in open(os.path.join(ROOT, "README.md")).read()


def test_importing_the_module_leaves_the_hyperparameters_alone():
    import hyperparams
    before = dict(hyperparams.DEFAULTS)
    from b2s_hip import variance  # noqa: F401
    assert hyperparams.DEFAULTS == before
    assert not [k for k in hyperparams.DEFAULTS if k.startswith("va_") or k.startswith("variance")]


def align256(v):
    return (v + 255) // 256 * 256


def test_host_side_refusals_come_back_as_messages_without_a_gpu():
    from b2s_hip import variance
    l = variance.load()

    def err():
        return l.b2s_va_last_error().decode()
    d = C.c_void_p(4096)                 # never dereferenced: every call below fails its checks before a launch
    odd = C.c_void_p(4096 + 8)           # 8-byte aligned only

    # the workspace formula of the header
    for B, S, D, nb in ((1, 1, 4, 1), (3, 5, 8, 2), (64, 128, 768, 256), (5, 257, 68, 256), (65535, 1, 4, 1)):
        assert l.b2s_va_ws_bytes(B, S, D, nb) == 16 + 2 * (align256(B * S * D * 4) + align256(B * nb * 4))
    for bad in (0, -1):
        assert l.b2s_va_ws_bytes(bad, 8, 8, 4) == 0 and "B must be > 0 (got %d)" % bad in err()
    assert l.b2s_va_ws_bytes(65536, 8, 8, 4) == 0 and "split the batch" in err()
    for bad in (0, 1025):
        assert l.b2s_va_ws_bytes(2, bad, 8, 4) == 0 and "S must be in 1..1024 (got %d)" % bad in err()
    for bad in (0, 6, 1028, -4):
        assert l.b2s_va_ws_bytes(2, 8, bad, 4) == 0 and "D must be a multiple of 4 in 4..1024 (got %d)" % bad in err()
    for bad in (0, 257):
        assert l.b2s_va_ws_bytes(2, 8, 8, bad) == 0 and "n_bins must be in 1..256 (got %d)" % bad in err()
    assert l.b2s_va_ws_bytes(65535, 1024, 1024, 4) == 0 and "sizes past one call" in err()
    assert l.b2s_va_ws_bytes(2048, 1024, 1024, 4) > 0                      # exactly 2^31 elements

    qg = dict(values=d, n_in=d, bounds=d, n_bins=8, B=2, S=16, bins=d, status=d)

    def quantise(**over):
        v = dict(qg, **over)
        return l.b2s_va_quantise(v["values"], v["n_in"], v["bounds"], v["n_bins"], v["B"], v["S"], v["bins"], v["status"], None)
    for bad in (0, -1):
        assert quantise(B=bad) != 0 and "B must be > 0 (got %d)" % bad in err()
    assert quantise(B=65536) != 0 and "split the batch" in err()
    for bad in (0, 1025):
        assert quantise(S=bad) != 0 and "S must be in 1..1024 (got %d)" % bad in err()
    for bad in (0, 257):
        assert quantise(n_bins=bad) != 0 and "n_bins must be in 1..256 (got %d)" % bad in err()
    for name in ("values", "n_in", "bins", "status"):
        assert quantise(**{name: None}) != 0 and "values, input_lengths, bins or status is NULL" in err()
    assert quantise(bounds=None) != 0 and "boundaries is NULL" in err()

    def frames(**over):
        v = dict(dict(dur=d, n_in=d, B=2, S=16, frames=d, status=d), **over)
        return l.b2s_va_frames(v["dur"], v["n_in"], v["B"], v["S"], v["frames"], v["status"], None)
    for bad in (0, -2):
        assert frames(B=bad) != 0 and "B must be > 0 (got %d)" % bad in err()
    assert frames(B=65536) != 0 and "split the batch" in err()
    for bad in (0, 1025):
        assert frames(S=bad) != 0 and "S must be in 1..1024 (got %d)" % bad in err()
    for name in ("dur", "n_in", "frames", "status"):
        assert frames(**{name: None}) != 0 and "durations, input_lengths, frames or status is NULL" in err()

    def pad(**over):
        v = dict(dict(frames=d, off=d, total=10, B=2, T=8, D=8, padded=d, to_frames=0, status=d), **over)
        return l.b2s_va_pad(v["frames"], v["off"], v["total"], v["B"], v["T"], v["D"], v["padded"], v["to_frames"], v["status"], None)
    for bad in (0, -2):
        assert pad(B=bad) != 0 and "B must be > 0 (got %d)" % bad in err()
    assert pad(B=65536) != 0 and "split the batch" in err()
    for bad in (0, (1 << 20) + 1):
        assert pad(T=bad) != 0 and "T must be in 1..1048576 (got %d)" % bad in err()
    for bad in (0, 6, 1028):
        assert pad(D=bad) != 0 and "D must be a multiple of 4 in 4..1024 (got %d)" % bad in err()
    assert pad(total=-1) != 0 and "total_frames must be >= 0 (got -1)" in err()
    assert pad(B=4096, T=1 << 20, D=8) != 0 and "sizes past one call" in err()
    for name in ("frames", "off", "padded", "status"):
        assert pad(**{name: None}) != 0 and "frames, frame_offsets, padded or status is NULL" in err()
    for name in ("frames", "padded"):
        assert pad(**{name: odd}) != 0 and "frames and padded must be 16-byte aligned" in err()

    fg = dict(x=d, pb=d, eb=d, pt=d, et=d, n_bins=8, dur=d, n_in=d, off=d, total=10, B=2, S=16, D=8, h=d, y=d, uof=d, status=d)

    def forward(**over):
        v = dict(fg, **over)
        return l.b2s_va_forward(v["x"], v["pb"], v["eb"], v["pt"], v["et"], v["n_bins"], v["dur"], v["n_in"], v["off"], v["total"],
                                v["B"], v["S"], v["D"], v["h"], v["y"], v["uof"], v["status"], None)
    need = l.b2s_va_ws_bytes(2, 16, 8, 8)
    bg = dict(dy=d, pb=d, eb=d, n_bins=8, dur=d, n_in=d, off=d, total=10, B=2, S=16, D=8, dx=d, dpt=d, det=d, status=d, ws=d,
              nbytes=need)

    def backward(**over):
        v = dict(bg, **over)
        return l.b2s_va_backward(v["dy"], v["pb"], v["eb"], v["n_bins"], v["dur"], v["n_in"], v["off"], v["total"], v["B"], v["S"],
                                 v["D"], v["dx"], v["dpt"], v["det"], v["status"], v["ws"], v["nbytes"], None)
    for call in (forward, backward):
        for bad in (0, -1):
            assert call(B=bad) != 0 and "B must be > 0 (got %d)" % bad in err()
        assert call(B=65536) != 0 and "split the batch" in err()
        for bad in (0, 1025):
            assert call(S=bad) != 0 and "S must be in 1..1024 (got %d)" % bad in err()
        for bad in (0, 6, 1028):
            assert call(D=bad) != 0 and "D must be a multiple of 4 in 4..1024 (got %d)" % bad in err()
        for bad in (0, 257):
            assert call(n_bins=bad) != 0 and "n_bins must be in 1..256 (got %d)" % bad in err()
        assert call(total=-1) != 0 and "total_frames must be >= 0 (got -1)" in err()
        assert call(B=65535, S=1024, D=1024) != 0 and "sizes past one call" in err()
        assert call(total=2 ** 31 - 1, D=1024) != 0 and "total_frames * D" in err() and "sizes past one call" in err()
        for name in ("dur", "n_in", "off", "status"):
            assert call(**{name: None}) != 0 and "durations, input_lengths, frame_offsets or status is NULL" in err()
    # a table without its bins, bins without their table
    assert forward(pb=None) != 0 and "the pitch table and pitch_bins are NULL together" in err()
    assert forward(pt=None) != 0 and "the pitch table and pitch_bins are NULL together" in err()
    assert forward(eb=None) != 0 and "the energy table and energy_bins are NULL together" in err()
    assert forward(et=None) != 0 and "the energy table and energy_bins are NULL together" in err()
    assert backward(pb=None) != 0 and "the pitch table and pitch_bins are NULL together" in err()
    assert backward(eb=None) != 0 and "the energy table and energy_bins are NULL together" in err()
    for name in ("x", "y"):
        assert forward(**{name: None}) != 0 and "x or y is NULL" in err()
    for name in ("dy", "dx"):
        assert backward(**{name: None}) != 0 and "dy or dx is NULL" in err()
    # 16-byte alignment of the fp32 arrays
    for name in ("x", "h", "y"):
        assert forward(**{name: odd}) != 0 and "x, h and y must be 16-byte aligned" in err()
    for name in ("pt", "et"):
        assert forward(**{name: odd}) != 0 and "tables must be 16-byte aligned" in err()
    for name in ("dy", "dx"):
        assert backward(**{name: odd}) != 0 and "dy and dx must be 16-byte aligned" in err()
    for name in ("dpt", "det"):
        assert backward(**{name: odd}) != 0 and "tables must be 16-byte aligned" in err()
    # the workspace
    assert backward(nbytes=need - 1) != 0 and "workspace of %d bytes, %d needed" % (need - 1, need) in err()
    assert backward(ws=None) != 0 and "workspace of 0 bytes, %d needed" % need in err()
    assert backward(ws=C.c_void_p(4098)) != 0 and "4-byte aligned" in err()


def test_there_is_no_cpu_fallback(monkeypatch):
    from b2s_hip import variance
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(variance.B2SError, match="runs on the GPU only"):
        variance.quantise_batch(np.zeros((1, 4)), [4], np.array([0.5]))
    with pytest.raises(variance.B2SError, match="runs on the GPU only"):
        variance.frame_counts(np.ones((1, 4), np.int32), [4])
    with pytest.raises(variance.B2SError, match="runs on the GPU only"):
        variance.expand(np.zeros((1, 4, 8), np.float32), np.ones((1, 4), np.int32), [4])
    va = variance.VarianceAdaptor(4, 8, [1.0, 2.0, 3.0], [1.0, 2.0, 3.0])
    assert sorted(n for n, _ in va.named_parameters()) == ["energy_embedding.weight", "pitch_embedding.weight"]
    assert sorted(n for n, _ in va.named_buffers()) == ["energy_boundaries", "pitch_boundaries"]
    assert va.pitch_embedding.weight.shape == (4, 8) and va.pitch_embedding.weight.dtype == torch.float32
    assert va.pitch_boundaries.dtype == torch.float64 and va.energy_boundaries.tolist() == [1.0, 2.0, 3.0]
    with pytest.raises(variance.B2SError, match="runs on the GPU only"):
        va(torch.zeros(1, 4, 8), np.zeros((1, 4)), np.zeros((1, 4)), np.ones((1, 4), np.int32), [4])
    with pytest.raises(variance.B2SError, match="2 boundaries for 4 bins"):
        variance.VarianceAdaptor(4, 8, [1.0, 2.0], [1.0, 2.0, 3.0])
    with pytest.raises(variance.B2SError, match="D must be a multiple of 4"):
        variance.VarianceAdaptor(4, 6, [1.0, 2.0, 3.0], [1.0, 2.0, 3.0])


# -------------------------------------------------------------------------------------------------- host-side Python functions

def test_boundaries_from_stats(tmp_path):
    from b2s_hip import variance
    stats = {"overall": {"pitch": {"count": 10, "mean": 150.0, "std": 30.0, "min": 50.0, "max": 450.0},
                         "energy": {"count": 10, "mean": 1.0, "std": 1.0, "min": 0.0, "max": 8.0},
                         "log_pitch": {"count": 0, "mean": None, "std": None, "min": None, "max": None}}}
    b = variance.boundaries_from_stats(stats, "pitch", 4)
    assert b.dtype == np.float64 and b.tolist() == [150.0, 250.0, 350.0]
    assert variance.boundaries_from_stats(stats, "energy", 8).tolist() == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]
    assert variance.boundaries_from_stats(stats, "pitch", 1).tolist() == []
    lg = variance.boundaries_from_stats(stats, "pitch", 2, scale="log")
    assert len(lg) == 1 and abs(lg[0] - 150.0) < 1e-9                      # the geometric mean of 50 and 450
    lg = variance.boundaries_from_stats(stats, "pitch", 256, scale="log")
    assert len(lg) == 255 and np.all(np.diff(lg) > 0) and 50.0 < lg[0] and lg[-1] < 450.0
    assert np.allclose(lg[1:] / lg[:-1], (450.0 / 50.0) ** (1 / 256.0))
    path = tmp_path / "stats.json"
    path.write_text(json.dumps(stats))
    assert variance.boundaries_from_stats(str(path), "pitch", 4).tolist() == [150.0, 250.0, 350.0]
    assert R.boundaries_ok(b) and R.boundaries_ok(lg)
    for args, text in ((("log_pitch", 4), "over 0 units"), (("nothing", 4), "no overall 'nothing'"), (("pitch", 0), "n_bins must be in"),
                       (("pitch", 257), "n_bins must be in"), (("energy", 4, "log"), "minimum above 0"), (("pitch", 4, "cubic"), "unknown scale")):
        with pytest.raises(variance.B2SError, match=text):
            variance.boundaries_from_stats(stats, *args)
    flat = {"overall": {"pitch": {"count": 3, "min": 100.0, "max": 100.0}}}
    with pytest.raises(variance.B2SError, match="do not ascend strictly"):
        variance.boundaries_from_stats(flat, "pitch", 4)
    assert variance.boundaries_from_stats(flat, "pitch", 1).tolist() == []


def test_padded_refuses_on_the_host_what_does_not_fit(monkeypatch):
    from b2s_hip import variance
    frames = torch.arange(1, 25, dtype=torch.float32).reshape(6, 4)
    with pytest.raises(variance.B2SError, match="does not fit T = 3"):
        variance.padded(frames, [0, 2, 2, 6], 3)
    with pytest.raises(variance.B2SError, match="do not pack 6 frames"):
        variance.padded(frames, [0, 2, 5], 5)
    with pytest.raises(variance.B2SError, match="fp32 tensor"):
        variance.padded(frames.double(), [0, 2, 2, 6], 5)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(variance.B2SError, match="runs on the GPU only"):
        variance.padded(frames, [0, 2, 2, 6], 5)


# ------------------------------------------------------------------------------------------------------------ the restatement

def integer_case(seed, B=3, S=9, D=8, n_bins=5):
    rng = np.random.default_rng(seed)
    x = rng.integers(-8, 9, size=(B, S, D)).astype(np.float32)
    pt = rng.integers(-8, 9, size=(n_bins, D)).astype(np.float32)
    et = rng.integers(-8, 9, size=(n_bins, D)).astype(np.float32)
    pb = rng.integers(0, n_bins, size=(B, S)).astype(np.int32)
    eb = rng.integers(0, n_bins, size=(B, S)).astype(np.int32)
    dur = rng.integers(0, 5, size=(B, S)).astype(np.int32)
    dur[0, 0] = dur[0, 3] = dur[0, 4] = 0
    n = np.array([S, S - 3, 1][:B] + [S] * max(0, B - 3), np.int32)
    off = R.offsets(dur, n)
    dy = rng.integers(-8, 9, size=(int(off[-1]), D)).astype(np.float32)
    return x, pt, et, pb, eb, dur, n, off, dy


@pytest.mark.parametrize("tables", ["both", "pitch", "energy", "none"])
def test_the_restatement_equals_torch_autograd_on_integers(tables):
    """Integers in -8..8: every sum below stays an integer far below 2^24, so fp32 is exact and the order of the additions cannot
    matter.  torch's CPU embedding, repeat_interleave and autograd are the independent ground."""
    x, pt, et, pb, eb, dur, n, off, dy = integer_case(11)
    if tables in ("energy", "none"):
        pt = pb = None
    if tables in ("pitch", "none"):
        et = eb = None
    total = int(off[-1])
    fw = R.forward(x, pb, eb, pt, et, dur, n, off, total)
    bw = R.backward(dy, pb, eb, 5, dur, n, off, total)
    assert fw["status"].tolist() == [R.OK] * 3 and bw["status"].tolist() == [R.OK] * 3
    tx = torch.from_numpy(x).requires_grad_(True)
    tp = None if pt is None else torch.from_numpy(pt).requires_grad_(True)
    te = None if et is None else torch.from_numpy(et).requires_grad_(True)
    rows, units = [], []
    for b in range(3):
        h = tx[b, :n[b]]
        if tp is not None:
            h = h + torch.nn.functional.embedding(torch.from_numpy(pb[b, :n[b]].astype(np.int64)), tp)
        if te is not None:
            h = h + torch.nn.functional.embedding(torch.from_numpy(eb[b, :n[b]].astype(np.int64)), te)
        reps = torch.from_numpy(dur[b, :n[b]].astype(np.int64))
        rows.append(torch.repeat_interleave(h, reps, dim=0))
        units.append(torch.repeat_interleave(torch.arange(int(n[b])), reps))
        assert np.array_equal(fw["h"][b, :n[b]], h.detach().numpy()) and not fw["h"][b, n[b]:].any()
    y = torch.cat(rows)
    assert np.array_equal(fw["y"], y.detach().numpy())
    assert np.array_equal(fw["unit_of_frame"], torch.cat(units).numpy())
    (y * torch.from_numpy(dy)).sum().backward()
    assert np.array_equal(bw["dx"], tx.grad.numpy())
    assert (bw["d_pitch_table"] is None) == (tp is None) and (bw["d_energy_table"] is None) == (te is None)
    if tp is not None:
        assert np.array_equal(bw["d_pitch_table"], tp.grad.numpy())
    if te is not None:
        assert np.array_equal(bw["d_energy_table"], te.grad.numpy())


def test_quantise_equals_bucketize_and_searchsorted():
    rng = np.random.default_rng(5)
    bd = np.sort(rng.normal(size=15))
    v = rng.normal(size=(3, 40))
    v[0, :15] = bd                                                         # exactly on a boundary: the bin below
    v[1, 0], v[1, 1], v[1, 2] = -np.inf, np.inf, bd[0]
    n = [40, 40, 17]
    bins, st = R.quantise(v, n, bd)
    assert st.tolist() == [R.OK] * 3
    want = torch.bucketize(torch.from_numpy(v), torch.from_numpy(bd), right=False).numpy()
    assert np.array_equal(want, np.searchsorted(bd, v, side="left"))
    for b in range(3):
        assert np.array_equal(bins[b, :n[b]], want[b, :n[b]]) and not bins[b, n[b]:].any()
    assert bins[0, :15].tolist() == list(range(15)) and bins[1, :3].tolist() == [0, 15, 0]
    one, st = R.quantise(v, n, None)                                       # one bin, no boundary
    assert not one.any() and st.tolist() == [R.OK] * 3


def test_the_statuses_of_the_restatement():
    bd = np.array([0.0, 1.0])
    v = np.array([[0.5, np.nan, 2.0], [0.5, 0.5, np.nan], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]])
    bins, st = R.quantise(v, [3, 2, 0, 4, -1], bd)
    assert st.tolist() == [R.FAILED, R.OK, R.EMPTY, R.FAILED, R.FAILED] and not bins[0].any() and bins[1].tolist() == [1, 1, 0]
    for bad in ([1.0, 1.0], [1.0, 0.0], [0.0, np.inf], [np.nan, 1.0]):
        bins, st = R.quantise(v, [1, 1, 1, 1, 1], np.array(bad))
        assert st.tolist() == [R.FAILED] * 5 and not bins.any()
    d = np.array([[1, 2, 3], [1, -1, 3], [R.MAX_FRAMES, 1, 0], [R.MAX_FRAMES, 0, 5], [4, 4, 4], [4, 4, 4]], np.int32)
    fr, st = R.frames(d, [3, 3, 2, 2, 0, 4])
    assert fr.tolist() == [6, 0, 0, R.MAX_FRAMES, 0, 0] and st.tolist() == [R.OK, R.FAILED, R.FAILED, R.OK, R.EMPTY, R.FAILED]
    assert fr.dtype == np.int32
    dur = np.array([[2, 1, 0]], np.int32)
    bins = np.array([[0, 4, 9]], np.int32)

    def one(n=3, dur=dur, bins=bins, off=(0, 3), total=3, n_bins=5):
        return int(R.statuses(bins, None, n_bins, dur, [n], off, total)[0]), int(R.statuses(None, bins, n_bins, dur, [n], off, total)[0])
    assert one(n=2) == (R.OK, R.OK)                                        # the bin of position 2 is not looked at
    assert one() == (R.FAILED, R.FAILED)                                   # bin 9 of 5
    assert one(n_bins=10) == (R.OK, R.OK)
    assert one(n=2, bins=np.array([[0, -1, 0]], np.int32)) == (R.FAILED, R.FAILED)
    assert one(n=4) == (R.FAILED, R.FAILED) and one(n=-1) == (R.FAILED, R.FAILED)
    assert one(n=2, dur=np.array([[2, -1, 0]], np.int32), off=(0, 1), total=1) == (R.FAILED, R.FAILED)
    assert one(n=2, off=(0, 2)) == (R.FAILED, R.FAILED)                    # one frame short
    assert one(n=2, off=(1, 4), total=3) == (R.FAILED, R.FAILED)           # leaves 0..total
    assert one(n=2, off=(3, 0), total=3) == (R.FAILED, R.FAILED)           # decreases
    assert one(n=0, off=(2, 2)) == (R.EMPTY, R.EMPTY)
    assert one(n=0, off=(0, 3)) == (R.FAILED, R.FAILED)                    # no position, three frames
    assert one(n=1, dur=np.array([[R.MAX_FRAMES + 1, 0, 0]], np.int32), off=(0, R.MAX_FRAMES + 1), total=R.MAX_FRAMES + 1) == (R.FAILED, R.FAILED)
    # what a FAILED or EMPTY utterance leaves behind
    x = np.ones((2, 3, 4), np.float32)
    fw = R.forward(x, None, None, None, None, np.array([[2, 1, 0], [1, 1, 1]], np.int32), [0, 3], [0, 0, 3], 3, sentinel=7.0)
    assert fw["status"].tolist() == [R.EMPTY, R.OK] and not fw["h"][0].any() and np.all(fw["y"] == 1.0)
    fw = R.forward(x, None, None, None, None, np.array([[2, -1, 0], [1, 1, 1]], np.int32), [3, 3], [0, 1, 4], 4, sentinel=7.0)
    assert fw["status"].tolist() == [R.FAILED, R.OK] and np.all(fw["h"][0] == 7.0) and np.all(fw["y"][0] == 7.0) and fw["unit_of_frame"].tolist() == [-1, 0, 1, 2]
    bw = R.backward(np.ones((4, 4), np.float32), np.zeros((2, 3), np.int32), None, 2, np.array([[2, -1, 0], [1, 1, 1]], np.int32), [3, 3],
                    [0, 1, 4], 4)
    assert not bw["dx"][0].any() and np.all(bw["dx"][1] == 1.0) and np.all(bw["d_pitch_table"][0] == 3.0) and not bw["d_pitch_table"][1].any()
    assert bw["d_energy_table"] is None


def test_a_minus_zero_survives_only_without_tables():
    x = np.full((1, 1, 4), -0.0, np.float32)
    dur, n, off = np.array([[2]], np.int32), [1], [0, 2]
    plain = R.forward(x, None, None, None, None, dur, n, off, 2)
    assert np.all(R.bits(plain["y"]) == np.int32(-2 ** 31))
    zero = np.zeros((1, 4), np.float32)
    with_table = R.forward(x, np.zeros((1, 1), np.int32), None, zero, None, dur, n, off, 2)
    assert np.all(R.bits(with_table["y"]) == 0)                            # -0.0 + +0.0 = +0.0: adding zero is not adding nothing
    bw = R.backward(np.full((2, 4), -0.0, np.float32), np.zeros((1, 1), np.int32), None, 1, dur, n, off, 2)
    assert np.all(R.bits(bw["dx"]) == 0) and np.all(R.bits(bw["d_pitch_table"]) == 0)      # a sum from +0.0 is never -0.0
