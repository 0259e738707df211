"""CPU-only tests of what the bindings share: the loader (b2s_hip.cbind.Library), the workspace and pointer helpers, the status words
and their raiser, the ragged-batch helpers (b2s_hip.ragged) and the opt-in switches (choice, rebind).  Nothing here needs a GPU."""
import ctypes as C
import sys
import types

import numpy as np
import pytest
import torch


def test_missing_library_raises_the_documented_text(tmp_path):
    from b2s_hip import cbind
    missing = cbind.Library("libb2s_nothing.so", {}, "b2s_nothing_last_error", path=str(tmp_path / "libb2s_nothing.so"))
    with pytest.raises(cbind.B2SError) as e:
        missing.load()
    assert str(e.value) == ("libb2s_nothing.so not found at %s -- build it with few-shot-transformer-tts_amd/csrc/build.sh "
                            "(or __graft_entry__.build()); there is no CPU fallback" % (tmp_path / "libb2s_nothing.so"))
    beside = cbind.Library("libb2s_nothing.so", {}, "b2s_nothing_last_error")
    assert beside.path.endswith("few-shot-transformer-tts_amd/libb2s_nothing.so") and beside.exports == []


def test_the_four_libraries_keep_their_module_level_names():
    from b2s_hip import B2SError, cbind, durations, f0, lib, mcd, metrics, vocoder
    assert lib.B2SError is cbind.B2SError is B2SError
    for mod, name in ((lib, "libb2s_hip.so"), (vocoder, "libb2s_vocoder.so"), (metrics, "libb2s_metrics.so"), (mcd, "libb2s_mcd.so"),
                      (f0, "libb2s_f0.so"), (durations, "libb2s_dur.so")):
        assert mod.LIB_PATH == mod._LIB.path and mod.LIB_PATH.endswith(name)
        assert mod.EXPORTS == mod._LIB.exports == sorted(mod._PROTOS) and mod._LIB.protos is mod._PROTOS
        assert mod.load() is mod.load()                                # cached
        assert mod.check(0) is None


def test_a_proto_the_library_lacks_is_an_attribute_error():
    from b2s_hip import cbind, mcd
    protos = dict(mcd._PROTOS, b2s_mcd_no_such_entry=(C.c_int, []))
    with pytest.raises(AttributeError, match="b2s_mcd_no_such_entry"):
        cbind.Library("libb2s_mcd.so", protos, "b2s_mcd_last_error").load()


def test_check_carries_the_message_of_its_own_library():
    """Each satellite library has an error slot of its own: a refusal of one does not show up in, or overwrite, another's.  (Both
    libraries word the refusal of B = 0 alike, so the MCD library is refused for its max_len here.)"""
    from b2s_hip import B2SError, mcd, metrics, vocoder
    assert mcd.load().b2s_mcd_ws_bytes(2, -1) == 0
    assert metrics.load().b2s_met_dtw_ws_bytes(0, 1, 1, 1, 1, 1, 1, 0) == 0
    assert vocoder.load().b2s_voc_silence_ws_bytes(1, 1, 2048, 512) == 0
    with pytest.raises(B2SError, match=r"^max_len must be >= 0 \(got -1\)$"):
        mcd.check(1)
    with pytest.raises(B2SError, match=r"^B must be > 0 \(got 0\)$"):
        metrics.check(1)
    with pytest.raises(B2SError, match=r"^silence_ws_bytes: Lmax must be >= 2 samples \(got 1\)"):
        vocoder.check(1)


def test_workspace_of_zero_bytes_raises_the_library_message():
    from b2s_hip import B2SError, mcd
    nbytes = mcd.load().b2s_mcd_ws_bytes(2, -1)
    assert nbytes == 0
    with pytest.raises(B2SError, match=r"max_len must be >= 0 \(got -1\)"):
        mcd.workspace(nbytes, "cpu")
    ws = mcd.workspace(mcd.load().b2s_mcd_ws_bytes(2, 100), "cpu")      # the helper only allocates: any torch device does
    assert ws.dtype == torch.uint8 and ws.numel() == mcd.load().b2s_mcd_ws_bytes(2, 100) > 0


def test_dptr_maps_none_and_on_request_empty_tensors_to_null():
    from b2s_hip.cbind import dptr
    t, empty = torch.zeros(3), torch.zeros(0)
    assert dptr(None) is None and dptr(None, empty_null=True) is None
    assert dptr(t).value == t.data_ptr() == dptr(t, empty_null=True).value
    assert dptr(empty, empty_null=True) is None and isinstance(dptr(empty), C.c_void_p)


def test_nptr_is_null_for_none_and_for_a_tensor_without_elements():
    from b2s_hip.cbind import nptr
    t = torch.zeros(3)
    assert nptr(None) is None and nptr(torch.zeros(0)) is None and nptr(torch.zeros(0, 4)) is None
    assert isinstance(nptr(t), C.c_void_p) and nptr(t).value == t.data_ptr() and nptr(t[1:]).value == t.data_ptr() + 4


def test_the_status_words_are_defined_once_and_shared():
    from b2s_hip import cbind, durations, f0, mcd, metrics
    assert (cbind.OK, cbind.EMPTY, cbind.FAILED) == (0, 1, 2)
    for mod in (metrics, mcd, f0, durations):
        assert (mod.OK, mod.EMPTY, mod.FAILED) == (0, 1, 2)
    assert durations.SHORT == 3 and durations.STATUS_NAMES == ("OK", "EMPTY", "FAILED", "SHORT")


def test_raise_failed_names_the_failed_items_in_each_of_the_three_texts():
    from b2s_hip.cbind import EMPTY, FAILED, OK, B2SError, raise_failed
    status = np.array([OK, FAILED, EMPTY, FAILED], np.int32)
    for args, kwargs, want in (
            (("DTW",), {}, "DTW failed for pairs [1, 3] (offsets inconsistent with the sizes)"),
            (("MCD after DTW", "utterances"), {}, "MCD after DTW failed for utterances [1, 3] (offsets inconsistent with the sizes)"),
            (("F0 after DTW",), {"why": "a non-finite sample, or sizes that do not fit together"},
             "F0 after DTW failed for pairs [1, 3] (a non-finite sample, or sizes that do not fit together)")):
        for st in (status, torch.from_numpy(status), status.tolist()):
            with pytest.raises(B2SError) as e:
                raise_failed(st, *args, **kwargs)
            assert str(e.value) == want
    for quiet in (np.array([OK, EMPTY, 3], np.int32), torch.tensor([OK, EMPTY], dtype=torch.int32), np.zeros(0, np.int32)):
        assert raise_failed(quiet, "DTW") is None


def test_default_hp_is_the_given_object_or_the_global_one():
    import hyperparams
    from b2s_hip.cbind import default_hp
    hp = types.SimpleNamespace()
    assert default_hp(hp) is hp and default_hp() is hyperparams.hparams and default_hp(None) is hyperparams.hparams


def test_ragged_as_tensor_detaches_a_tensor_and_wraps_anything_else():
    from b2s_hip import ragged
    w = torch.ones(3, requires_grad=True) * 2.0
    t = ragged.as_tensor(w)
    assert w.requires_grad and not t.requires_grad and t.data_ptr() == w.data_ptr()
    a = np.arange(6, dtype=np.int16).reshape(2, 3)
    t = ragged.as_tensor(a)
    assert t.dtype == torch.int16 and t.tolist() == a.tolist()
    a[0, 0] = 7
    assert t[0, 0] == 7                                                # the array's memory, not a copy
    assert ragged.as_tensor([1.5, 2.5]).dtype == torch.float64 and ragged.as_tensor([[1, 2]]).shape == (1, 2)


def test_ragged_lengths_i32():
    from b2s_hip import B2SError, ragged
    for given, want in (([3, 0, 7], [3, 0, 7]), (torch.tensor([3, 0, 7], dtype=torch.int64), [3, 0, 7]),
                        (np.array([[3], [0], [7]]), [3, 0, 7]),                                    # any shape of B values
                        (np.array([2.9, -1.9, 7.0]), [2, -1, 7]), (torch.tensor([2.9, -1.9, 7.0]), [2, -1, 7]),
                        ([1000000, -5, 0], [1000000, -5, 0])):                                     # nothing is clamped
        t = ragged.lengths_i32(given, 3, "cpu", "input_lengths")
        assert t.dtype == torch.int32 and t.is_contiguous() and t.tolist() == want
    assert ragged.lengths_i32([], 0, "cpu", "dec_lengths").shape == (0,)
    for given in ([3, 0], torch.tensor([3, 0]), np.array([3.0, 0.0])):
        with pytest.raises(B2SError, match="^2 dec_lengths for a batch of 3$"):
            ragged.lengths_i32(given, 3, "cpu", "dec_lengths")


def test_ragged_offsets():
    from b2s_hip import B2SError, ragged
    for lengths, want in (([], [0]), ([0], [0, 0]), ([3, 0, 2], [0, 3, 3, 5])):
        off = ragged.offsets(lengths)
        assert off.dtype == np.int32 and off.tolist() == want
    off, off_d = ragged.offsets([3, 0, 2], "cpu")
    assert off.tolist() == [0, 3, 3, 5] and off_d.dtype == torch.int32 and off_d.tolist() == [0, 3, 3, 5]
    assert ragged.offsets([2 ** 30, 2 ** 30 - 1]).tolist() == [0, 2 ** 30, 2 ** 31 - 1]       # the largest total int32 holds
    with pytest.raises(B2SError, match="^2147483648 symbols in one batch: the offsets are int32$"):
        ragged.offsets([2 ** 30, 2 ** 30])


def test_ragged_pack_lengths_and_batches():
    from b2s_hip import B2SError, ragged
    x = np.zeros((2, 5, 3), np.float32)
    packed, off = ragged.pack(ragged.as_batch(x + np.arange(5)[None, :, None], "cpu", "x"), [3, 2])
    assert packed.shape == (5, 3) and off.tolist() == [0, 3, 5] and packed[:, 0].tolist() == [0, 1, 2, 0, 1]
    assert off.dtype == np.int32 and packed.dtype == torch.float32 and packed.is_contiguous()
    assert tuple(ragged.as_batch(np.zeros((2, 5)), "cpu", "x").shape) == (2, 5, 1)
    with pytest.raises(B2SError, match=r"x must be \[B, T, dim\] or \[B, T\]"):
        ragged.as_batch(np.zeros(5), "cpu", "x")
    assert ragged.lengths(torch.tensor([7, 2]), 2, 5, "x") == [5, 2]
    out = {"path": torch.tensor([[0, 0], [1, 1], [9, 9], [0, 0]], dtype=torch.int32), "path_len": torch.tensor([2, 0, 1]),
           "path_offsets": np.array([0, 3, 3, 4], np.int32)}
    paths = ragged.paths(out)
    assert [p.tolist() for p in paths] == [[[0, 0], [1, 1]], [], [[0, 0]]] and all(p.dtype == np.int64 for p in paths)


def test_ragged_device_prefers_a_tensor_that_is_on_a_device():
    from b2s_hip import B2SError, ragged
    if torch.cuda.is_available():
        assert ragged.device("the test", np.zeros(1), torch.zeros(1)).type == "cuda"
    else:
        with pytest.raises(B2SError, match="^the test runs on the GPU only; no HIP device is visible$"):
            ragged.device("the test", np.zeros(1), torch.zeros(1))


def test_choice_and_rebind_round_trip(monkeypatch):
    from b2s_hip.cbind import choice, rebind
    hp = types.SimpleNamespace(knob="reference")
    assert choice(hp, "knob") == "reference"
    hp.knob = "hip"
    assert choice(hp, "knob") == "hip"
    hp.knob = "scipy"
    with pytest.raises(ValueError, match=r"^unknown knob 'scipy' \(expected 'reference' or 'hip'\)$"):
        choice(hp, "knob")

    def original():
        return "original"

    def replacement():
        return "replacement"
    slot = "_b2s_reference_thing"
    assert rebind("b2s_stand_in", "thing", replacement, slot, True) is False              # the module is not imported
    stand_in = types.ModuleType("b2s_stand_in")
    monkeypatch.setitem(sys.modules, "b2s_stand_in", stand_in)
    assert rebind("b2s_stand_in", "thing", replacement, slot, True) is False              # the module lacks the attribute
    stand_in.thing = original
    assert rebind("b2s_stand_in", "thing", replacement, slot, False) is False and stand_in.thing is original
    assert rebind("b2s_stand_in", "thing", replacement, slot, True) is True
    assert stand_in.thing is replacement and getattr(stand_in, slot) is original
    assert rebind("b2s_stand_in", "thing", replacement, slot, True) is False              # idempotent: the slot keeps the original
    assert stand_in.thing is replacement and getattr(stand_in, slot) is original
    assert rebind("b2s_stand_in", "thing", replacement, slot, False) is True
    assert stand_in.thing is original and not hasattr(stand_in, slot)
    assert rebind("b2s_stand_in", "thing", replacement, slot, False) is False
