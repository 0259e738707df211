"""The GPU edit distance (b2s_met_edit_distance of libb2s_metrics.so, b2s_hip.cer) against the host restatements of its contract
(tests/edit_ref.py).  Every result is an integer, so every comparison is exact: distance, substitutions, deletions, insertions and
status.  The shapes sit on the kernel's edges: strips of 1..64 columns per lane, lanes without a column, the result in a lane other
than the last, fewer truth symbols than lanes, empty sides, the 4096-symbol limit."""
import json

import numpy as np
import pytest
import torch

import edit_ref as R

pytestmark = pytest.mark.gpu

OK, FAILED = 0, 2


def offsets(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.int32)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return off


def flat(seqs):
    parts = [np.asarray(s, dtype=np.int32) for s in seqs]
    return np.concatenate(parts + [np.zeros(1, np.int32)])             # never empty; the extra symbol lies past every offset


def raw(a_seqs, b_seqs, want_ops=True, a_off=None, b_off=None, max_a=None, max_b=None):
    """One call of the C ABI; host arrays (dist [B], ops [B, 3] or None, status [B])."""
    from b2s_hip import metrics
    lib = metrics.load()
    dev = torch.device("cuda")
    a_off = offsets(a_seqs) if a_off is None else np.asarray(a_off, dtype=np.int32)
    b_off = offsets(b_seqs) if b_off is None else np.asarray(b_off, dtype=np.int32)
    B = len(a_off) - 1
    total_a, total_b = sum(len(s) for s in a_seqs), sum(len(s) for s in b_seqs)
    max_a = max(len(s) for s in a_seqs) if max_a is None else max_a
    max_b = max(len(s) for s in b_seqs) if max_b is None else max_b
    a, b = torch.from_numpy(flat(a_seqs)).to(dev), torch.from_numpy(flat(b_seqs)).to(dev)
    ao, bo = torch.from_numpy(a_off).to(dev), torch.from_numpy(b_off).to(dev)
    dist = torch.full((B,), -7, dtype=torch.int32, device=dev)
    ops = torch.full((B, 3), -7, dtype=torch.int32, device=dev) if want_ops else None
    status = torch.full((B,), -7, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    metrics.check(lib.b2s_met_edit_distance(a.data_ptr(), ao.data_ptr(), total_a, max_a, b.data_ptr(), bo.data_ptr(), total_b, max_b,
                                            B, dist.data_ptr(), ops.data_ptr() if want_ops else None, status.data_ptr(), stream))
    torch.cuda.synchronize()
    return dist.cpu().numpy(), ops.cpu().numpy() if want_ops else None, status.cpu().numpy()


def expect(a_seqs, b_seqs):
    rows = np.asarray([R.edit_packed(a, b) for a, b in zip(a_seqs, b_seqs)], dtype=np.int64).reshape(len(a_seqs), 4)
    return rows[:, 0], rows[:, 1:]


def check_batch(a_seqs, b_seqs):
    dist, ops, status = raw(a_seqs, b_seqs)
    want_d, want_o = expect(a_seqs, b_seqs)
    assert status.tolist() == [OK] * len(a_seqs)
    bad = [i for i in range(len(a_seqs)) if dist[i] != want_d[i] or ops[i].tolist() != want_o[i].tolist()]
    assert not bad, [(i, len(a_seqs[i]), len(b_seqs[i]), int(dist[i]), ops[i].tolist(), int(want_d[i]), want_o[i].tolist())
                     for i in bad[:5]]


def shaped_pairs():
    rng = np.random.default_rng(77)

    def seq(n, k=12):
        return rng.integers(k, size=n).astype(np.int32)
    pairs = [(seq(0), seq(0)), (seq(0), seq(5)), (seq(5), seq(0)),
             (np.array([3], np.int32), np.array([3], np.int32)), (np.array([3], np.int32), np.array([4], np.int32))]
    for la, lb in ((1, 64), (64, 1), (63, 65), (64, 64), (65, 63), (128, 129), (129, 128), (200, 7), (7, 200)):
        pairs.append((seq(la), seq(lb)))
    pairs.append((seq(300, 3), seq(300, 3)))                          # three symbols: many ties between alignments
    pairs += [(seq(1000), seq(37)), (seq(37), seq(1000))]
    same = seq(500)
    pairs.append((same, same.copy()))
    pairs.append((seq(500, 6), seq(500, 6) + 100))                     # no symbol in common: 500 substitutions
    return [p[0] for p in pairs], [p[1] for p in pairs]


def test_shapes_on_every_edge_of_the_kernel():
    a, b = shaped_pairs()
    assert len(a) == 19
    check_batch(a, b)
    dist, ops, _ = raw(a, b)
    assert dist[-2] == 0 and ops[-2].tolist() == [0, 0, 0]
    assert dist[-1] == 500 and ops[-1].tolist() == [500, 0, 0]
    assert ops[1].tolist() == [0, 0, 5] and ops[2].tolist() == [0, 5, 0]


def test_every_strip_width_takes_its_own_path():
    """max_b picks the launch's widest strip and each pair its own: one short and one full-width pair for every width 1..64."""
    rng = np.random.default_rng(5)
    for width in (1, 2, 4, 8, 16, 32):
        lb = 64 * width - 3
        a = [rng.integers(4, size=70).astype(np.int32), rng.integers(4, size=90).astype(np.int32)]
        b = [rng.integers(4, size=33).astype(np.int32), rng.integers(4, size=lb).astype(np.int32)]
        check_batch(a, b)


def test_longest_pair_and_the_swap_symmetry():
    rng = np.random.default_rng(11)
    a, b = rng.integers(4, size=4096).astype(np.int32), rng.integers(4, size=4095).astype(np.int32)
    cost, sub, dele, ins = R.edit_packed(a, b)
    dist, ops, status = raw([a, b], [b, a])
    assert status.tolist() == [OK, OK]
    assert dist.tolist() == [cost, cost]
    assert ops[0].tolist() == [sub, dele, ins] and ops[1].tolist() == [sub, ins, dele]


def test_symbols_are_compared_as_whole_int32_values():
    vals = np.array([-1, 0, 0x10FFFF, 2 ** 31 - 1, -2 ** 31, 0x10000, 1], dtype=np.int32)
    rng = np.random.default_rng(3)
    a = [vals[rng.integers(len(vals), size=n)] for n in (40, 90, 7)]
    b = [vals[rng.integers(len(vals), size=n)] for n in (45, 80, 7)]
    check_batch(a, b)


def test_one_pair_and_513_pairs():
    rng = np.random.default_rng(9)
    check_batch([rng.integers(5, size=23).astype(np.int32)], [rng.integers(5, size=31).astype(np.int32)])
    a = [rng.integers(6, size=int(rng.integers(0, 40))).astype(np.int32) for _ in range(513)]
    b = [rng.integers(6, size=int(rng.integers(0, 40))).astype(np.int32) for _ in range(513)]
    check_batch(a, b)


def test_ops_are_optional_and_runs_are_bit_identical():
    rng = np.random.default_rng(21)
    a = [rng.integers(8, size=int(rng.integers(50, 300))).astype(np.int32) for _ in range(40)]
    b = [R.mutate(rng, s, 0.1, 8) for s in a]
    d0, o0, s0 = raw(a, b)
    d1, o1, s1 = raw(a, b)
    d2, none, s2 = raw(a, b, want_ops=False)
    assert none is None
    assert np.array_equal(d0, d1) and np.array_equal(o0, o1) and np.array_equal(s0, s1)
    assert np.array_equal(d0, d2) and np.array_equal(s0, s2)
    assert np.array_equal(d0, expect(a, b)[0])


def test_inconsistent_pairs_fail_alone():
    rng = np.random.default_rng(31)
    a = [rng.integers(5, size=n).astype(np.int32) for n in (20, 30, 10, 25, 12)]
    b = [rng.integers(5, size=n).astype(np.int32) for n in (22, 28, 40, 25, 9)]
    a_off, b_off = offsets(a), offsets(b)
    a_off[2] -= 35                       # pair 1 now ends before it starts (decreasing offsets); pair 2 grows to 45 <= max_a
    want_d, want_o = expect([a[0], flat(a)[a_off[2]:a_off[3]], a[3], a[4]], [b[0], b[2], b[3], b[4]])
    dist, ops, status = raw(a, b, a_off=a_off, b_off=b_off, max_a=64, max_b=39)          # pair 2's prediction (40) exceeds max_b
    assert status.tolist() == [OK, FAILED, FAILED, OK, OK]
    assert dist[1] == -1 and dist[2] == -1 and ops[1].tolist() == [-1] * 3 and ops[2].tolist() == [-1] * 3
    keep = [0, 3, 4]
    assert dist[keep].tolist() == want_d[[0, 2, 3]].tolist() and ops[keep].tolist() == want_o[[0, 2, 3]].tolist()
    # offsets past the total, and a negative first offset, fail too; nothing is read through them
    a_off2 = offsets(a)
    a_off2[5] += 1000
    b_off2 = offsets(b)
    b_off2[0] = -4
    _, _, status = raw(a, b, a_off=a_off2, b_off=b_off2, max_a=4096, max_b=4096)
    assert status.tolist() == [FAILED, OK, OK, OK, FAILED]


# ---------------------------------------------------------------------------------------------------------------- through Python

def test_python_input_kinds_and_errors():
    from b2s_hip import cer
    truths = ["kitten", b"\x00abc", np.array([5, 6, 7], np.int64), ["the", "cat", "sat"], "", "aé\U0001F600"]
    preds = ["sitting", b"abc\xff", [5, 7], ["the", "dog", "sat", "down"], "xy", "ae\U0001F600"]
    dist, ops = cer.edit_distance_batch(truths, preds, return_ops=True)
    assert dist.is_cuda and dist.dtype == torch.int32 and tuple(ops.shape) == (6, 3)
    assert dist.tolist() == [3, 2, 1, 2, 2, 1]
    assert ops.tolist() == [[2, 0, 1], [0, 1, 1], [0, 1, 0], [1, 0, 1], [0, 0, 2], [1, 0, 0]]
    assert cer.edit_distance_batch(truths, preds).tolist() == dist.tolist()
    assert cer.eval("kitten", "sitting") == 3
    packed = cer.pack(truths[:1]), cer.pack(preds[:1])
    assert cer.edit_distance_batch(*packed).tolist() == [3]
    with pytest.raises(cer.B2SError, match="at most 4096"):
        cer.edit_distance_batch(["a" * 4097], ["a"])
    with pytest.raises(cer.B2SError, match="2 truths for 1 predictions"):
        cer.edit_distance_batch(["a", "b"], ["a"])


def test_cer_batch_equals_the_reference_formula():
    from b2s_hip import cer
    rng = np.random.default_rng(41)
    truths = ["".join(chr(0x61 + int(v)) for v in rng.integers(20, size=int(rng.integers(0, 60)))) for _ in range(50)]
    preds = ["".join(chr(int(v)) for v in R.mutate(rng, [ord(c) for c in t], 0.3, 0x7A) if v >= 0x20) for t in truths]
    preds[3], truths[4] = "", ""
    want = [R.cer(R.edit_packed([ord(c) for c in t], [ord(c) for c in p])[0], len(p)) for t, p in zip(truths, preds)]
    got = cer.cer_batch(truths, preds)
    assert got == want and all(type(v) is float for v in got)


def test_score_transcriptions_equals_the_host_computation(tmp_path):
    from b2s_hip import cer
    rng = np.random.default_rng(51)
    locales = ["en-us", "zh-cn", "ko-kr"]
    records = []
    for i in range(30):
        if i in (7, 19):
            records.append({"name": "s%02d" % i, "locale": locales[i % 3], "cer": 1.0, "DisplayText": "", "fail": True})
            continue
        truth = "".join(chr(0x4E00 + int(v)) for v in rng.integers(30, size=int(rng.integers(5, 40))))
        pred = "".join(chr(int(v)) for v in R.mutate(rng, [ord(c) for c in truth], 0.2, 0x4E00 + 30))
        records.append({"name": "s%02d" % i, "locale": locales[i % 3], "truth": truth, "pred": pred, "DisplayText": pred, "cer": 0.0})
    path = tmp_path / "transcriptions.jsonl"
    path.write_text("".join(json.dumps(r, ensure_ascii=False) + "\n" for r in records), encoding="utf-8")
    res = cer.score_transcriptions(str(path))
    cers, per = [], {}
    for r in records:
        if "fail" in r:
            cers.append(1.0)
            continue
        c, s, d, n = R.edit_packed([ord(ch) for ch in r["truth"]], [ord(ch) for ch in r["pred"]])
        cers.append(R.cer(c, len(r["pred"])))
        acc = per.setdefault(r["locale"], {"vals": [], "dist": 0, "sub": 0, "del": 0, "ins": 0, "truth_len": 0, "pred_len": 0})
        acc["vals"].append(cers[-1])
        for k, v in (("dist", c), ("sub", s), ("del", d), ("ins", n), ("truth_len", len(r["truth"])), ("pred_len", len(r["pred"]))):
            acc[k] += v
    assert res["cers"] == cers and res["raw_cer"] == float(np.mean(cers)) and res["n_failed"] == 2
    assert set(res["locales"]) == set(per)
    for loc, acc in per.items():
        got = res["locales"][loc]
        assert got["n"] == len(acc["vals"]) and got["cer"] == sum(acc["vals"]) / len(acc["vals"])
        assert got["micro_cer"] == acc["dist"] / acc["pred_len"]
        assert all(got[k] == acc[k] for k in ("sub", "del", "ins", "truth_len", "pred_len"))
