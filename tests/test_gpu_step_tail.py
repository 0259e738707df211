"""The tail of a training step per element against the float64 restatement tests/step_tail_ref.py: the loss (b2s_loss_forward: k_loss_partial_v,
k_loss_finalize), its gradient (b2s_loss_backward), the L2 term on both routes (k_mt_sumsq; the per-chunk sums of squares a full Adam step leaves,
k_sum_scaled) and its gradient (b2s_l2_backward), and the fused multi-tensor Adam (k_mt_adam2 through b2s_adam_step / b2s_adam_step_groups /
b2s_adam_set_grad_wire) with its bf16 shadows and conv images.  The tests write the inputs, the gradients (eng._gflat) and the moments
(trainer.exp_avg / exp_avg_sq) themselves and call the C entry points directly; no model backward runs.  Every comparison is over all elements.

Bars: step_tail_ref's docstring (derived ones counted from the kernel text; measured ones 4 x the worst error of this file's cases, capped by the project's
scalar bar).  tests/test_step_tail_ref_host.py checks the checker on the CPU.  Every test prints what it measured; with B2S_TEST_RECORD_DIR set the worst
values go to r14_step_tail_parity.json there (committed copy: profiles/)."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import synth, TINY, TINY96
from gpu_util import DEV
from test_gpu_model import build, dev_batch
import step_tail_ref as R

RECORD = "r14_step_tail_parity.json"
CHUNK = 16384                  # elements per chunk of the multi-tensor tables (engine.hip: build_chunks)
TAIL_WORKGROUPS = 512          # grid cap of b2s_adam_step_groups(behind_mark = 1)
F32 = lambda x: float(np.float32(x))
LR, EPS = F32(1e-3), F32(5e-8)
# decoder group above 512 chunks: the capped grid's workgroups take a second chunk (cix += gridDim.x)
BIG = ("vocab_size=260,embed_size=512,encoder_hidden=512,decoder_hidden=768,speaker_embedding_size=128,language_embedding_size=128,"
       "n_attention_head=8,n_encoder_layer=1,n_decoder_layer=1,prenet_hidden=32,postnet_hidden=48,n_postnet_layer=2,max_num_speaker=8,"
       "max_num_language=8,transformer_dropout_rate=0.0,decoder_dropout_rate=0.0")


def record(section, values, how=max):
    """values {key: number} merged into the record file's `section` (worst value per key)."""
    out_dir = os.environ.get("B2S_TEST_RECORD_DIR")
    if not out_dir:
        return
    try:
        os.makedirs(out_dir, exist_ok=True)
        path = os.path.join(out_dir, RECORD)
        data = json.load(open(path)) if os.path.exists(path) else {}
        s = data.setdefault(section, {})
        for k, v in values.items():
            s[k] = how(s[k], v) if k in s else v
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


class Rig(object):
    """A model with an attached HipTrainer, and its parameters / gradients / moments as flat host arrays in the layout of the flat gradient buffer."""

    def __init__(self, over, dtype="fp32"):
        from b2s_hip import lib as L
        from b2s_hip.trainer import HipTrainer
        self.L = L
        self.m, self.cfg, self.st, self.hp = build(over, compute_dtype=dtype)
        self.tr = HipTrainer(self.m, self.hp, dist=False)
        self.eng, self.lib = self.tr.eng, self.tr.lib
        self.h = self.eng.handle
        self.params = dict(self.m.named_parameters())
        self.offs = dict(self.eng.param_offsets)
        assert set(self.offs) == set(self.params)
        self.n = self.eng._gflat.numel()
        self.member = np.zeros(self.n, dtype=bool)
        for k, (o, c) in self.offs.items():
            self.member[o:o + c] = R.l2_member(k)
        self.rw = F32(self.cfg.reg_weight)

    def seeded(self, seed=0):
        """(p, g, m, v) flat fp32, step_tail_ref.adam_inputs per tensor; zeros in the padding between the tensors' slots."""
        flat = [np.zeros(self.n, dtype=np.float32) for _ in range(4)]
        for k, (o, c) in self.offs.items():
            for dst, a in zip(flat, R.adam_inputs(k, c, seed)):
                dst[o:o + c] = a
        return flat

    def put(self, p=None, g=None, m=None, v=None):
        with torch.no_grad():
            if p is not None:
                for k, (o, c) in self.offs.items():
                    self.params[k].data.copy_(torch.from_numpy(p[o:o + c]).view(self.params[k].shape))
            for dst, a in ((self.eng._gflat, g), (self.tr.exp_avg, m), (self.tr.exp_avg_sq, v)):
                if a is not None:
                    dst.copy_(torch.from_numpy(a))

    def masters(self):
        p = np.zeros(self.n, dtype=np.float32)
        for k, (o, c) in self.offs.items():
            p[o:o + c] = self.params[k].detach().cpu().numpy().reshape(-1)
        return p

    def get(self):
        torch.cuda.synchronize()
        return self.masters(), self.tr.exp_avg.cpu().numpy(), self.tr.exp_avg_sq.cpu().numpy()

    def by_name(self, flat):
        return {k: flat[o:o + c] for k, (o, c) in self.offs.items()}

    def name_at(self, i):
        for k, (o, c) in self.offs.items():
            if o <= i < o + c:
                return "%s[%d]" % (k, i - o)
        return "padding[%d]" % i

    def adam_step(self, lr, step, l2, gs):
        self.L.check(self.lib.b2s_adam_step(self.h, lr, step, R.BETA1, R.BETA2, EPS, l2, gs, self.L.stream()))

    def l2_now(self):
        return R.l2_value(self.by_name(self.masters()), self.rw)

    def loss_forward(self, dev, B, T, dirty=True):
        """b2s_loss_forward on device tensors dev = (bef, aft, stop, tgt, lens32) with the scratch buffer pre-filled with 1e30 -> (out[7], aft_losses[B])."""
        L = self.L
        vals = torch.full((7,), float("nan"), device=DEV)
        per = torch.full((B,), float("nan"), device=DEV)
        scratch = torch.full((8 + B,), 1e30 if dirty else 0.0, device=DEV)
        L.check(self.lib.b2s_loss_forward(self.h, *(L.ptr(t) for t in dev), B, T, L.ptr(vals), L.ptr(per), L.ptr(scratch), L.stream()))
        torch.cuda.synchronize()
        return vals.cpu().numpy(), per.cpu().numpy()


def check_adam(rig, tag, got, s0, hyper, member=None, where=None):
    """every element of p', m', v' against the float64 restatement at the derived bars; -> (worst error in bars per kind, number of elements that
    differ bit-wise from the float32 restatement)."""
    member = rig.member if member is None else member
    ref = R.adam(*s0, *hyper, member)
    bars = R.adam_bars(*s0, *hyper, member)
    r32 = R.adam(*s0, *hyper, member, dtype=np.float32)
    worst, nbits = {}, 0
    for kind, a, r, b, r3 in zip("pmv", got, ref, bars, r32):
        sel = slice(None) if where is None else where
        a, r, b, r3 = a[sel], r[sel], b[sel], r3[sel]
        assert np.isfinite(a).all(), (tag, kind)
        d = np.abs(a.astype(np.float64) - r)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(d == 0, 0.0, d / b)
        i = int(np.argmax(q))
        worst[kind] = float(q[i])
        assert q[i] <= 1.0, (tag, kind, rig.name_at(i) if where is None else i, float(a[i]), float(r[i]), float(d[i]), float(b[i]))
        nbits += int((a.view(np.uint32) != r3.view(np.uint32)).sum())
    return worst, nbits


# ===================================================================================================================== loss
_LOSS_RIGS = {}


def loss_rig(num_mels):
    if num_mels not in _LOSS_RIGS:
        _LOSS_RIGS[num_mels] = Rig(TINY + ",num_mels=%d" % num_mels)
    return _LOSS_RIGS[num_mels]


@pytest.mark.parametrize("route", ["recompute", "l2_fresh"])
@pytest.mark.parametrize("case", list(R.LOSS_CASES))
def test_loss_and_gradients_vs_fp64(case, route):
    """The seven loss values, aft_losses and the three gradients, element by element, on a scratch buffer full of 1e30.  recompute: the L2 term is
    read from the parameters (k_mt_sumsq).  l2_fresh: directly after a full b2s_adam_step it comes from the per-chunk sums of squares the update
    left (k_sum_scaled, which also has to clear the loss accumulators)."""
    C_, B, T, _ = R.LOSS_CASES[case]
    rig = loss_rig(C_)
    L = rig.L
    bef, aft, stop, tgt, lens = R.loss_inputs(case)
    dev = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (bef, aft, stop, tgt)) + (torch.from_numpy(lens.astype(np.int32)).to(DEV),)
    rig.put(*rig.seeded())
    if route == "recompute":
        L.check(rig.lib.b2s_model_sync_weights(rig.h, L.stream(), 0))
    else:
        rig.adam_step(LR, 1, rig.rw, 1.0)
    out, per = rig.loss_forward(dev, B, T)
    l2 = rig.l2_now()
    ro, rper = R.loss(bef, aft, stop, tgt, lens, l2)
    ex = R.loss_excess({"out": out, "aft_losses": per}, {"out": ro, "aft_losses": rper})
    e = abs(float(out[4]) - l2) / l2
    ex["l2/" + route] = (e / R.BAR_L2, e)
    if route == "l2_fresh":                      # the next call recomputes from the parameters: same masters, same value
        L.check(rig.lib.b2s_model_sync_weights(rig.h, L.stream(), 0))
        out2, _ = rig.loss_forward(dev, B, T)
        assert abs(float(out2[4]) - l2) / l2 <= R.BAR_L2 and abs(float(out2[0]) - float(out[0])) <= 2 * R.BAR_SCALAR * abs(float(ro[0]))
    pad = ~R._valid(lens, T)
    for w3 in R.W3:
        d = [torch.full_like(dev[0], float("nan")), torch.full_like(dev[0], float("nan")), torch.full_like(dev[2], float("nan"))]
        w = None if w3 is None else torch.tensor(w3, dtype=torch.float32, device=DEV)
        L.check(rig.lib.b2s_loss_backward(rig.h, *(L.ptr(t) for t in dev), B, T, L.ptr(w), *(L.ptr(t) for t in d), L.stream()))
        torch.cuda.synchronize()
        got = dict(zip(("d_bef", "d_aft", "d_stop"), (t.cpu().numpy() for t in d)))
        ref = dict(zip(("d_bef", "d_aft", "d_stop"), R.loss_grads(bef, aft, stop, tgt, lens, w3)), lens=lens)
        for k, g in got.items():
            assert np.isfinite(g).all() and not g[pad].any(), (case, k)                      # padded rows exactly 0.0
        assert not got["d_bef"][bef == tgt].any()
        for k, v in R.loss_excess(got, ref, w3).items():
            ex[k] = max(ex.get(k, (0.0, 0.0)), v)
    print("%s / %s: " % (case, route) + ", ".join("%s %.3g (%.3f bars)" % (k, v[1], v[0]) for k, v in sorted(ex.items())))
    record("measured_worst", {k: v[1] for k, v in ex.items()})
    record("bars", {"scalar": R.BAR_SCALAR, "aft_losses": R.BAR_AFT_LOSSES, "l2": R.BAR_L2, "d_stop": R.BAR_DSTOP, "d_bef": R.BAR_DMEL, "d_aft": R.BAR_DMEL})
    bad = {k: v for k, v in ex.items() if not v[0] <= 1.0}
    assert not bad, (case, route, bad)


@pytest.mark.parametrize("gscale", [None, 0.5])
def test_l2_backward_members_only(gscale):
    """b2s_l2_backward adds reg_weight gscale p to the gradients of the L2 members; every other element of the flat gradient buffer (non-members
    and the padding between the slots) stays bit-identical."""
    rig = loss_rig(80)
    L = rig.L
    p, g, m, v = rig.seeded()
    rig.put(p, g, m, v)
    gs = None if gscale is None else torch.tensor([gscale], dtype=torch.float32, device=DEV)
    L.check(rig.lib.b2s_l2_backward(rig.h, L.ptr(gs), L.stream()))
    torch.cuda.synchronize()
    got = rig.eng._gflat.cpu().numpy()
    mem = rig.member
    assert np.array_equal(got[~mem].view(np.uint32), g[~mem].view(np.uint32))
    a = rig.rw * (1.0 if gscale is None else gscale)
    ref = g.astype(np.float64) + a * p.astype(np.float64)
    bar = R.BAR_L2_BWD * R.SLACK * (np.abs(g.astype(np.float64)) + np.abs(a * p.astype(np.float64)))
    d = np.abs(got.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d == 0, 0.0, d / bar)[mem]
    print("l2 backward, gscale %s: %d member elements, worst %.3f bars" % (gscale, int(mem.sum()), float(q.max())))
    record("derived_worst_in_bars", {"l2_backward": float(q.max())})
    assert mem.sum() > 0 and float(q.max()) <= 1.0
    assert (got[mem] != g[mem]).any()


# ===================================================================================================================== Adam
def adam_cases(rig):
    return list(itertools.product(R.ADAM_STEPS, R.ADAM_SCALES, (0.0, rig.rw, F32(0.1))))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("tag", ["tiny", "tiny96"])
def test_adam_step_every_element_vs_fp64(tag, dtype):
    """One b2s_adam_step from a seeded state, step in {1, 7, 100000} x grad_scale in {1, 0.5} x l2 in {0, reg_weight, 0.1}: every element of every
    parameter, exp_avg and exp_avg_sq.  l2 = 0.1 moves members and non-members apart by far more than a bar: the member set, tensor by tensor."""
    rig = Rig({"tiny": TINY, "tiny96": TINY96}[tag], dtype)
    s0 = rig.seeded()
    worst, nbits = {}, {}
    for step, gs, l2 in adam_cases(rig):
        rig.put(*s0)
        rig.adam_step(LR, step, l2, gs)
        key = "%s/%s step=%d gs=%g l2=%g" % (tag, dtype, step, gs, l2)
        w, nb = check_adam(rig, key, rig.get(), s0, (LR, step, R.BETA1, R.BETA2, EPS, l2, gs))
        nbits[key] = nb
        for k, x in w.items():
            worst[k] = max(worst.get(k, 0.0), x)
    print("%s/%s: worst element in bars %s; elements differing bit-wise from the float32 restatement: %d of %d per case at most"
          % (tag, dtype, worst, max(nbits.values()), 3 * rig.n))
    record("derived_worst_in_bars", {"adam_" + k: x for k, x in worst.items()})
    record("adam_bitwise_differences", {"%s/%s (%d cases)" % (tag, dtype, len(nbits)): sum(nbits.values())})
    if R.ADAM_BITWISE:
        assert not any(nbits.values()), {k: x for k, x in nbits.items() if x}


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_adam_reads_the_bf16_gradient_wire(dtype):
    """b2s_adam_set_grad_wire: the gradients come from a bf16 buffer laid out like the flat gradient buffer; that buffer itself holds NaN."""
    rig = Rig(TINY, dtype)
    L = rig.L
    p, g, m, v = rig.seeded()
    gw = R.bf16_rne(g)
    wire = torch.from_numpy(gw).to(DEV).to(torch.bfloat16)
    assert np.array_equal(wire.float().cpu().numpy(), gw) and (gw != g).any()
    rig.put(p, np.full_like(g, np.nan), m, v)
    hyper = (LR, 7, R.BETA1, R.BETA2, EPS, rig.rw, 0.5)
    L.check(rig.lib.b2s_adam_set_grad_wire(rig.h, L.ptr(wire), L.ptr(rig.eng._gflat)))
    try:
        rig.adam_step(LR, 7, rig.rw, 0.5)
        got = rig.get()
    finally:
        L.check(rig.lib.b2s_adam_set_grad_wire(rig.h, None, None))
    w, nb = check_adam(rig, "wire/" + dtype, got, (p, gw, m, v), hyper)
    print("bf16 wire / %s: worst element in bars %s, %d bit-wise differences" % (dtype, w, nb))
    record("derived_worst_in_bars", {"adam_wire_" + k: x for k, x in w.items()})
    record("adam_bitwise_differences", {"wire/" + dtype: nb})
    if R.ADAM_BITWISE:
        assert nb == 0
    # ... and without the wire the same call reads the flat buffer again
    rig.put(p, g, m, v)
    rig.adam_step(LR, 7, rig.rw, 0.5)
    check_adam(rig, "wire unset/" + dtype, rig.get(), (p, g, m, v), hyper)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_adam_frozen_encoder(dtype):
    """freeze_encoder: one step leaves every encoder parameter and moment bit-identical; the L2 value of the next loss still includes the encoder's
    members (read from the parameters: the chunk sums of the update do not cover them)."""
    rig = Rig(TINY + ",freeze_encoder=true", dtype)
    s0 = rig.seeded()
    rig.put(*s0)
    rig.adam_step(LR, 7, rig.rw, 1.0)
    got = rig.get()
    enc = np.zeros(rig.n, dtype=bool)
    for k, (o, c) in rig.offs.items():
        enc[o:o + c] = k.startswith("encoder.")
    assert enc.any() and (~enc).any()
    for a, b in zip(got, s0[:1] + s0[2:]):
        assert np.array_equal(a[enc].view(np.uint32), b[enc].view(np.uint32))
    w, _ = check_adam(rig, "frozen/" + dtype, got, s0, (LR, 7, R.BETA1, R.BETA2, EPS, rig.rw, 1.0), where=~enc)
    moved = float((got[0][~enc] != s0[0][~enc]).mean())
    assert moved > 0.5, moved
    bef, aft, stop, tgt, lens = R.loss_inputs("golden")
    dev = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (bef, aft, stop, tgt)) + (torch.from_numpy(lens.astype(np.int32)).to(DEV),)
    out, _ = rig.loss_forward(dev, 3, 23)
    l2 = rig.l2_now()
    without = R.l2_value({k: x for k, x in rig.by_name(got[0]).items() if not k.startswith("encoder.")}, rig.rw)
    e = abs(float(out[4]) - l2) / l2
    print("frozen encoder / %s: worst element in bars %s; l2 %.6g (rel. error %.2e; without the encoder's members %.6g)" % (dtype, w, l2, e, without))
    record("measured_worst", {"l2/frozen": e})
    assert e <= R.BAR_L2 and abs(without - l2) / l2 > 1e-2                      # (the encoder's share is 100 bars and more)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_adam_groups_and_capped_grid(dtype):
    """b2s_adam_step_groups: decoder + postnet behind the mark on the capped grid (more than 512 decoder chunks: second trip of the chunk loop), then
    the encoder: bit-identical to one b2s_adam_step from the same state and within the bars of float64; the encoder is untouched in between; the L2
    value of the next loss comes from the chunk sums of all three groups."""
    rig = Rig(BIG, dtype)
    L = rig.L
    chunks = {}
    for k, (o, c) in rig.offs.items():
        chunks[k.split(".")[0]] = chunks.get(k.split(".")[0], 0) + -(-c // CHUNK)
    print("chunks per group: %s" % chunks)
    assert chunks["decoder"] > TAIL_WORKGROUPS, chunks
    s0 = rig.seeded()
    hyper = (LR, 7, R.BETA1, R.BETA2, EPS, rig.rw, 0.5)
    args = (rig.h, LR, 7, R.BETA1, R.BETA2, EPS, rig.rw, 0.5)
    enc = np.zeros(rig.n, dtype=bool)
    for k, (o, c) in rig.offs.items():
        enc[o:o + c] = k.startswith("encoder.")
    rig.put(*s0)
    L.check(rig.lib.b2s_model_mark_grads_ready(rig.h))
    L.check(rig.lib.b2s_adam_step_groups(*args, 2 | 4, 1, L.stream()))
    mid = rig.get()
    for a, b in zip(mid, s0[:1] + s0[2:]):
        assert np.array_equal(a[enc].view(np.uint32), b[enc].view(np.uint32))
    assert float((mid[0][~enc] != s0[0][~enc]).mean()) > 0.5
    L.check(rig.lib.b2s_adam_step_groups(*args, 1, 0, L.stream()))
    grouped = rig.get()
    bef, aft, stop, tgt, lens = R.loss_inputs("golden")
    dev = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (bef, aft, stop, tgt)) + (torch.from_numpy(lens.astype(np.int32)).to(DEV),)
    out, _ = rig.loss_forward(dev, 3, 23)
    l2 = R.l2_value(rig.by_name(grouped[0]), rig.rw)
    e = abs(float(out[4]) - l2) / l2
    rig.put(*s0)
    rig.adam_step(LR, 7, rig.rw, 0.5)
    whole = rig.get()
    for kind, a, b in zip("pmv", grouped, whole):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), kind
    w, nb = check_adam(rig, "groups/" + dtype, whole, s0, hyper)
    print("groups / %s: worst element in bars %s, %d bit-wise differences; l2 after the grouped step: rel. error %.2e" % (dtype, w, nb, e))
    record("derived_worst_in_bars", {"adam_groups_" + k: x for k, x in w.items()})
    record("adam_bitwise_differences", {"groups/" + dtype: nb})
    record("measured_worst", {"l2/groups": e})
    assert e <= R.BAR_L2
    if R.ADAM_BITWISE:
        assert nb == 0


# ===================================================================================================================== shadows and conv images
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_shadows_and_conv_images_follow_the_update(dtype):
    """No accessor reads the bf16 shadows or the conv images, so they are checked through what reads them.  After a step with lr = 0.05 (every bf16
    value moves) the eval forward of the whole model (shadows, forward conv image) and a train-mode postnet forward + backward (backward conv image:
    x.grad) must not change bit-wise when b2s_model_sync_weights(.., 0) re-derives shadows and images from the masters -- and must differ from before
    the step.  The compared outputs are deterministic call to call (checked first): all five in bf16 mode, all but the postnet's x.grad in fp32 mode,
    where the images are re-laid out behind the update."""
    rig = Rig(TINY96, dtype)
    L, m, cfg = rig.L, rig.m, rig.cfg
    b = dev_batch(synth.synthetic_batch(cfg, B=3, S=11, T=23, seed=7, in_lens=[11, 7, 4], tgt_lens=[23, 15, 9]))
    g = torch.Generator().manual_seed(11)
    x, go = torch.randn(3, 23, cfg.num_mels, generator=g).to(DEV), torch.randn(3, 23, cfg.num_mels, generator=g).to(DEV)

    def run():
        m.eval()
        with torch.no_grad():
            o = m(**b)
        res = [o[k].detach().clone() for k in ("mel_bef", "mel_aft", "stop_logits")]
        m.postnet.train()
        stats = {k: v.detach().clone() for k, v in m.postnet.named_buffers()}         # (the train-mode forward moves the running statistics the eval forward reads)
        xd = x.clone().requires_grad_(True)
        po = m.postnet(xd, b["target_lengths"])
        po.backward(go)
        with torch.no_grad():
            for k, v in m.postnet.named_buffers():
                v.copy_(stats[k])
        torch.cuda.synchronize()
        return res + [po.detach().clone(), xd.grad.clone()]

    names = ("mel_bef", "mel_aft", "stop_logits", "postnet out", "postnet x.grad")
    before, again = run(), run()
    if dtype == "fp32":
        # the fp32 postnet backward is not deterministic call to call (its x.grad differs in the last bits between two identical calls), so in fp32
        # mode the backward image is left to tests/test_gpu_postnet.py; it is written by the same relayout kernel before and after the re-sync anyway
        names = names[:4]
    for k, a, c in zip(names, before, again):
        assert torch.equal(a, c), "%s is not deterministic call to call" % k
    _, g0, _, _ = rig.seeded()
    g0 = np.where(g0 == 0, np.float32(1e-3), g0)
    rig.put(None, g0, np.zeros_like(g0), np.zeros_like(g0))
    rig.adam_step(F32(0.05), 1, rig.rw, 1.0)
    after = run()
    L.check(rig.lib.b2s_model_sync_weights(rig.h, L.stream(), 0))
    resync = run()
    for k, a, c, z in zip(names, after, resync, before):
        assert torch.isfinite(a).all(), k
        assert torch.equal(a, c), "%s changes when shadows / images are re-derived from the masters: max |d| = %.3g" % (k, float((a - c).abs().max()))
        assert not torch.equal(a, z), k
