"""CPU-only tests of the CER feature's host side: the b2s_met_edit_* C ABI (declared, exported, bound; every host-side refusal
without a GPU), basic_normalize against the recorded outputs of the reference (tests/golden/g10_cer.json), the two restatements of
the edit-distance contract (tests/edit_ref.py) against each other, cer_batch / score_transcriptions with the restatement standing in
for the kernel, and the `cer` hyper-parameter with install()."""
import ctypes as C
import json
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import edit_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fresh_hp(over=""):
    import hyperparams
    hp = hyperparams.hparams
    hp.override_from_dict(hyperparams.DEFAULTS)
    if over:
        hp.parse(over)
    return hp


# --------------------------------------------------------------------------------------------------------------------- the C ABI

NEW_SYMBOLS = ("b2s_met_edit_max_len", "b2s_met_edit_distance")


def test_new_symbols_are_declared_exported_and_bound():
    from b2s_hip import cer, metrics
    l = metrics.load()
    header = open(os.path.join(ROOT, "include", "b2s_metrics.h")).read()
    declared = set(re.findall(r"\b(b2s_met_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    for name in NEW_SYMBOLS:
        assert name in metrics.EXPORTS and name in metrics._PROTOS and name in declared and hasattr(l, name)
    assert len(metrics.EXPORTS) == 9
    assert l.b2s_met_edit_max_len() == 4096 and cer.max_len() == 4096


def test_host_side_refusals_come_back_as_messages_without_a_gpu():
    from b2s_hip import metrics
    l = metrics.load()

    def err():
        return l.b2s_met_last_error().decode()
    d = C.c_void_p(16)                   # never dereferenced: every call below fails its checks before a launch
    good = dict(a=d, ao=d, ta=10, ma=5, b=d, bo=d, tb=10, mb=5, B=2, dist=d, ops=None, status=d)

    def call(**over):
        v = dict(good, **over)
        return l.b2s_met_edit_distance(v["a"], v["ao"], v["ta"], v["ma"], v["b"], v["bo"], v["tb"], v["mb"], v["B"], v["dist"],
                                       v["ops"], v["status"], None)
    for bad in (0, -1):
        assert call(B=bad) != 0 and "B must be > 0 (got %d)" % bad in err()
    assert call(ta=-1) != 0 and "totals must be >= 0" in err()
    assert call(tb=-7) != 0 and "totals must be >= 0" in err()
    for bad in (-1, 4097):
        assert call(ma=bad) != 0 and "max_a must be in 0..4096 (got %d)" % bad in err()
        assert call(mb=bad) != 0 and "max_b must be in 0..4096 (got %d)" % bad in err()
    assert call(ao=None) != 0 and "a_offsets or b_offsets is NULL" in err()
    assert call(bo=None) != 0 and "a_offsets or b_offsets is NULL" in err()
    assert call(a=None) != 0 and "a or b is NULL" in err()
    assert call(b=None) != 0 and "a or b is NULL" in err()
    assert call(dist=None) != 0 and "dist_out or status_out is NULL" in err()
    assert call(status=None) != 0 and "dist_out or status_out is NULL" in err()


# ----------------------------------------------------------------------------------------------------------- the normalisation

def test_basic_normalize_equals_the_recorded_reference_outputs(golden_dir):
    from b2s_hip import cer
    cases = json.load(open(os.path.join(golden_dir, "g10_cer.json")))["cases"]
    assert len(cases) >= 40
    locales = {c["locale"] for c in cases}
    assert {"zh", "zh-cn", "th-th", "zh-tw", "zh-hk", "ja-jp", "ko-kr", "en-us"} <= locales
    for c in cases:
        assert [ord(ch) for ch in cer.basic_normalize(c["text"], c["locale"])] == c["out"], c


# ----------------------------------------------------------------------------------------------------------- the restatements

def test_the_two_restatements_agree_on_500_seeded_pairs():
    rng = np.random.default_rng(20240612)
    for n in range(500):
        k = (2, 3, 5)[n % 3]
        a = rng.integers(k, size=int(rng.integers(0, 21)))
        b = rng.integers(k, size=int(rng.integers(0, 21)))
        t, p = R.edit_tuples(a, b), R.edit_packed(a, b)
        assert t == p, (a, b, t, p)
        assert t[0] == t[1] + t[2] + t[3] and t[2] - t[3] == len(a) - len(b)


def test_restatement_on_cases_known_by_hand():
    as_ints = lambda s: [ord(c) for c in s]                                   # noqa: E731
    assert R.edit_packed(as_ints("kitten"), as_ints("sitting")) == (3, 2, 0, 1)
    assert R.edit_packed(as_ints("abc"), []) == (3, 0, 3, 0)
    assert R.edit_packed([], as_ints("abc")) == (3, 0, 0, 3)
    assert R.edit_packed([], []) == (0, 0, 0, 0)
    assert R.edit_packed(as_ints("ab"), as_ints("ba")) == (2, 0, 1, 1)          # two substitutions cost the same: fewer subs win


# ------------------------------------------------------------------------------------- scoring, with the restatement as the kernel

def _host_batch(truths, preds, return_ops=False):
    """edit_distance_batch's contract on the host (CPU tensors), through the module's own symbol conversion."""
    from b2s_hip import cer
    vocab = {}
    rows = [R.edit_packed(cer._symbols(t, vocab), cer._symbols(p, vocab)) for t, p in zip(truths, preds)]
    dist = torch.tensor([r[0] for r in rows], dtype=torch.int32)
    ops = torch.tensor([r[1:] for r in rows], dtype=torch.int32).reshape(len(rows), 3)
    return (dist, ops) if return_ops else dist


def test_cer_batch_formula(monkeypatch):
    from b2s_hip import cer
    monkeypatch.setattr(cer, "edit_distance_batch", _host_batch)
    got = cer.cer_batch(["abc", "", "", "kitten"], ["", "abc", "", "sitting"])
    assert got == [1.0, 3 / (3 + 1e-9), 0.0, 3 / (7 + 1e-9)]
    assert all(type(v) is float for v in got)
    assert cer.eval("kitten", "sitting") == 3 and type(cer.eval("a", "b")) is int


RECORDS = [
    {"name": "a1", "locale": "en-us", "truth": "hello world", "pred": "hello word", "DisplayText": "x", "cer": 0.5},
    {"name": "a2", "locale": "en-us", "truth": "abc", "pred": "abc", "DisplayText": "x", "cer": 0.5},
    {"name": "a3", "locale": "en-us", "truth": "abcdef", "pred": "ab", "DisplayText": "x", "cer": 0.5},
    {"name": "k1", "locale": "ko-kr", "truth": "kitten", "pred": "sitting", "DisplayText": "x", "cer": 0.5},
    {"name": "k2", "locale": "ko-kr", "cer": 1.0, "DisplayText": "", "fail": True},
]


def test_score_transcriptions_on_a_hand_written_jsonl(monkeypatch, tmp_path):
    from b2s_hip import cer
    monkeypatch.setattr(cer, "edit_distance_batch", _host_batch)
    path = tmp_path / "transcriptions.jsonl"
    path.write_text("".join(json.dumps(r, ensure_ascii=False) + "\n" for r in RECORDS), encoding="utf-8")
    c = [1 / (10 + 1e-9), 0.0, 1.0, 3 / (7 + 1e-9)]            # a3: 4 deletions over 2 predicted symbols, capped at 1.0
    for source in (str(path), RECORDS):
        res = cer.score_transcriptions(source)
        assert res["n"] == 5 and res["n_failed"] == 1
        assert res["cers"] == c + [1.0]
        assert res["raw_cer"] == float(np.mean(c + [1.0]))
        assert list(res["locales"]) == ["en-us", "ko-kr"]
        en, ko = res["locales"]["en-us"], res["locales"]["ko-kr"]
        assert en["n"] == 3 and en["cer"] == (0 + c[0] + c[1] + c[2]) / 3
        assert en["micro_cer"] == (1 + 0 + 4) / (10 + 3 + 2)
        assert (en["sub"], en["del"], en["ins"], en["truth_len"], en["pred_len"]) == (0, 5, 0, 20, 15)
        assert ko["n"] == 1 and ko["cer"] == c[3] and ko["micro_cer"] == 3 / 7           # the failed record is not in the window
        assert (ko["sub"], ko["del"], ko["ins"], ko["truth_len"], ko["pred_len"]) == (2, 0, 1, 6, 7)


def test_score_transcriptions_renormalize(monkeypatch):
    from b2s_hip import cer
    monkeypatch.setattr(cer, "edit_distance_batch", _host_batch)
    recs = [{"name": "r1", "locale": "en-us", "truth": "stale", "pred": "stale!", "meta": {"t": "Hello, World!"},
             "NBest": [{"Lexical": "hello  world"}]},
            {"name": "r2", "locale": "zh-cn", "truth": "你 好", "pred": "你好"}]
    assert cer.score_transcriptions(recs)["cers"] == [1 / (6 + 1e-9), 1 / (2 + 1e-9)]
    assert cer.score_transcriptions(recs, renormalize=True)["cers"] == [0.0, 0.0]


def test_command_line_prints_the_summary(monkeypatch, tmp_path, capsys):
    from b2s_hip import cer
    monkeypatch.setattr(cer, "edit_distance_batch", _host_batch)
    path = tmp_path / "transcriptions.jsonl"
    path.write_text("".join(json.dumps(r) + "\n" for r in RECORDS), encoding="utf-8")
    out = tmp_path / "summary.json"
    assert cer.main([str(path), "--json", str(out)]) == 0
    printed = json.loads(capsys.readouterr().out)
    assert printed["locales"]["ko-kr"]["sub"] == 2 and "cers" not in printed
    assert json.load(open(out))["cers"][-1] == 1.0


def test_symbol_conversion_of_every_input_kind():
    from b2s_hip import cer
    vocab = {}
    assert cer._symbols("aé\U0001F600", vocab).tolist() == [0x61, 0xE9, 0x1F600]
    assert cer._symbols(b"\x00\xff", vocab).tolist() == [0, 255]
    assert cer._symbols(np.array([-1, 2 ** 31 - 1], dtype=np.int64), vocab).tolist() == [-1, 2 ** 31 - 1]
    assert cer._symbols([], vocab).tolist() == [] and cer._symbols("", vocab).tolist() == []
    assert cer._symbols(["the", "cat", "the"], vocab).tolist() == [0, 1, 0]
    assert cer._symbols(["dog", "cat"], vocab).tolist() == [2, 1]                # one dict for both sides of a call
    for bad in (np.zeros((2, 2), np.int32), np.zeros(3, np.float32), np.array([2 ** 31], dtype=np.int64)):
        with pytest.raises(cer.B2SError):
            cer._symbols(bad, vocab)


def test_there_is_no_cpu_fallback(monkeypatch):
    from b2s_hip import cer
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(cer.B2SError, match="runs on the GPU only"):
        cer.edit_distance_batch(["kitten"], ["sitting"])


# ------------------------------------------------------------------------------------------------------------ hyper-parameter

def test_cer_hparam_defaults_to_reference_and_parses_hip():
    import hyperparams
    hp = fresh_hp()
    assert hp.cer == "reference" and hyperparams.DEFAULTS["cer"] == "reference"
    hp.parse("cer=hip")
    try:
        assert hp.cer == "hip"
    finally:
        fresh_hp()


def test_install_binds_restores_and_refuses(monkeypatch):
    from b2s_hip import cer
    original = types.ModuleType("editdistance")
    original.eval = lambda a, b: -1
    fake = types.ModuleType("utils.transcribe")
    fake.editdistance = original
    monkeypatch.setitem(sys.modules, "utils.transcribe", fake)
    try:
        cer.install(fresh_hp())                                   # default: nothing is touched
        assert fake.editdistance is original and not hasattr(fake, cer._ORIGINAL)
        cer.install(fresh_hp("cer=hip"))
        assert fake.editdistance is not original and fake.editdistance.eval is cer.eval
        cer.install(fresh_hp("cer=hip"))                          # twice: the original is kept, not overwritten by the stand-in
        assert getattr(fake, cer._ORIGINAL) is original
        cer.install(fresh_hp())
        assert fake.editdistance is original and not hasattr(fake, cer._ORIGINAL)
        with pytest.raises(ValueError, match="unknown cer 'foo'"):
            cer.install(fresh_hp("cer=foo"))
        assert fake.editdistance is original
    finally:
        fresh_hp()


def test_install_without_the_reference_module_is_a_no_op(monkeypatch):
    from b2s_hip import cer
    monkeypatch.delitem(sys.modules, "utils.transcribe", raising=False)
    try:
        cer.install(fresh_hp("cer=hip"))
        assert "utils.transcribe" not in sys.modules
    finally:
        fresh_hp()


def test_eval_batch_refuses_an_unknown_cer_before_any_work():
    import synthesize

    class Boom(object):
        def engine(self):
            raise RuntimeError("stand-in model: never reached")
    fresh_hp("cer=foo")
    try:
        with pytest.raises(ValueError, match="unknown cer 'foo'"):
            synthesize.eval_batch(Boom(), {"inputs": np.zeros((1, 3))})
    finally:
        fresh_hp()
