"""GPU tests: edge-case shapes against the oracle, and the data-parallel trainer with 2 ranks sharing one GPU
(gloo backend over device tensors -- RCCL refuses two ranks on one device; the driver's multi-GPU bench uses nccl)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "few-shot-transformer-tts_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import b2s_oracle as O            # noqa: E402  (checker only)
from oracle import synth, make_config, TINY    # noqa: E402

DEV = "cuda"


def _build(over, seed=1234, compute_dtype="fp32"):
    from hyperparams import hparams as hp
    from transformer.tacotron import Tacotron
    import hyperparams
    hp.override_from_dict(hyperparams.DEFAULTS)
    hp.parse(over)
    hp.parse("compute_dtype=%s" % compute_dtype)
    cfg = make_config(over)
    m = Tacotron(hp)
    st = synth.synthetic_state(cfg, seed)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in st.items()}, strict=True)
    return m.to(DEV), cfg, st, hp


def _dev(nb):
    return {k: (torch.from_numpy(np.asarray(v)).to(DEV) if not isinstance(v, list) else v) for k, v in nb.items()}


@pytest.mark.parametrize("B,S,T,in_lens,tgt_lens", [
    (1, 5, 9, [5], [9]),                      # single utterance
    (2, 3, 2, [3, 2], [2, 1]),                # minimal lengths (target length 1: stop target on frame 0)
    (3, 70, 131, [70, 1 + 1, 33], [131, 64, 1]),      # ragged, tiles straddle 64/128 boundaries
    (2, 130, 257, [130, 65], [257, 129]),     # > 2 attention tiles in both directions
])
def test_edge_shapes_forward_backward(B, S, T, in_lens, tgt_lens):
    from transformer.tacotron import compute_loss
    m, cfg, st, hp = _build(TINY)
    nb = synth.synthetic_batch(cfg, B=B, S=S, T=T, seed=B * 31 + T, in_lens=in_lens, tgt_lens=tgt_lens)
    b = _dev(nb)
    m.train()
    o = m(**b)
    losses = compute_loss(m, b["mel_targets"], b["target_lengths"], o, hp)
    losses["loss"].backward()
    torch.cuda.synchronize()
    P = O.to_torch_state(st, requires_grad=True)
    ob = O.to_torch_batch(nb)
    ro = O.tacotron_forward(P, cfg, ob, train=True)
    rl = O.compute_loss(P, cfg, ob["mel_targets"], ob["target_lengths"], ro)
    names = [n for n in P if O.is_parameter(n)]
    grads = torch.autograd.grad(rl["loss"], [P[n] for n in names], allow_unused=True)
    for k in ("mel_bef", "mel_aft", "stop_logits"):
        d = float((o[k].detach().cpu() - ro[k].detach()).abs().max())
        assert d < 3e-4, (k, d)
    assert abs(float(losses["loss"]) - float(rl["loss"])) < 1e-4 * max(1.0, abs(float(rl["loss"])))
    al = o["alignments"]["encdec"][1].cpu()
    assert float((al - ro["alignments"]["encdec"][1].detach()).abs().max()) < 1e-5
    got = dict(m.named_parameters())
    for n, g in zip(names, grads):
        ref = g if g is not None else torch.zeros_like(P[n])
        err = float((got[n].grad.cpu() - ref).abs().max())
        assert err < 3e-4 * max(1.0, float(ref.norm())), (n, err)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _dp_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from b2s_hip.trainer import HipTrainer
    torch.manual_seed(0)
    m, cfg, st, hp = _build(TINY, seed=1234 if rank == 0 else 999)      # rank 1 starts different: the trainer must broadcast rank 0's
    m.train()
    tr = HipTrainer(m, hp, bucket_mb=0.05, grad_payload="fp32")     # exact mean of the rank gradients (HipTrainer's default wire; bench.py selects the bf16 wire for its bf16 lines)
    assert tr.world == 2 and tr.bucketer is not None and tr.bn_broadcast
    for step in range(2):
        nb = synth.synthetic_batch(cfg, B=2, S=9, T=14, seed=100 + 10 * step + rank)
        vals = tr.train_step(_dev(nb))
        assert len(tr.bucketer.launched) > 1
    torch.cuda.synchronize()
    sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **sd)
    dist.destroy_process_group()


def test_data_parallel_trainer_two_ranks(tmp_path):
    """2 ranks: identical parameters afterwards, equal to the oracle's mean-of-rank-gradients Adam steps."""
    import torch.multiprocessing as mp
    port = _free_port()
    mp.spawn(_dp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0 = dict(np.load(os.path.join(str(tmp_path), "rank0.npz")))
    r1 = dict(np.load(os.path.join(str(tmp_path), "rank1.npz")))
    cfg = make_config(TINY)
    P = O.to_torch_state(synth.synthetic_state(cfg, 1234), requires_grad=True)
    opt = {}
    names = [n for n in P if O.is_parameter(n)]
    for step in range(2):
        gsum = None
        for rank in range(2):
            ob = O.to_torch_batch(synth.synthetic_batch(cfg, B=2, S=9, T=14, seed=100 + 10 * step + rank))
            o = O.tacotron_forward(P, cfg, ob, train=True)
            loss = O.compute_loss(P, cfg, ob["mel_targets"], ob["target_lengths"], o)["loss"]
            g = torch.autograd.grad(loss, [P[n] for n in names], allow_unused=True)
            g = [x if x is not None else torch.zeros_like(P[n]) for x, n in zip(g, names)]
            gsum = g if gsum is None else [a + b for a, b in zip(gsum, g)]
        with torch.no_grad():
            O.adam_step(P, {n: x / 2 for n, x in zip(names, gsum)}, opt, step, cfg)
    for n in names:
        assert np.array_equal(r0[n], r1[n]), n                      # replicas stay bit-identical
        ref = P[n].detach().numpy()
        assert abs(np.linalg.norm(r0[n]) - np.linalg.norm(ref)) <= 2e-4 * np.linalg.norm(ref) + 1e-5, n
        assert np.abs(r0[n] - ref).max() < 4.5e-3, n               # <= 2 steps x lr on ill-conditioned (|g|~0) elements


def test_rccl_exchange_path_single_rank():
    """The production exchange path on RCCL itself (backend "nccl", one rank -- RCCL refuses two ranks on one device):
    process-group init with device_id, asynchronous all-reduce launched from the engine's stage hook, work.wait(),
    barrier and MAX-reduce of bench.py.  Same seeds => same loss as the run without a process group."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--full", "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
           "--no-roofline-pass", "--batch", "4", "--S", "40", "--T", "120"]
    outs = []
    for force in (True, False):
        env = dict(os.environ)
        env.pop("B2S_FORCE_DP", None)
        if force:
            env.update(B2S_FORCE_DP="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), RANK="0", WORLD_SIZE="1")
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        outs.append(json.loads(lines[0]))
    assert outs[0]["n_gpus"] == 1 and np.isfinite(outs[0]["final_loss"])
    # bf16 + dropout + fp32-atomic conv weight gradients: runs are not bit-reproducible, a few steps differ by ~1e-3
    assert abs(outs[0]["final_loss"] - outs[1]["final_loss"]) < 1e-2 * abs(outs[1]["final_loss"])
    # the data-parallel line decides the defaults in ONE invocation: every (dp_mode, wire) leg, the exchange path with the wire removed and the
    # no-process-group step, each timed and finite, plus what the first SCALE run reads off them
    d = outs[0]
    assert d["rccl_ranks"] == 1 and "dp_legs" not in outs[1]
    legs = {l["leg"]: l for l in d["dp_legs"]}
    assert len(legs) == 6 and all("error" not in l and l["ms_per_step"] > 0 for l in legs.values()), d["dp_legs"]
    assert {(l["dp_mode"], l["wire"]) for l in legs.values() if l["dp_mode"]} == {("allreduce", "fp32"), ("allreduce", "bf16"), ("rs_ag", "fp32"), ("rs_ag", "bf16")}
    assert all(np.isfinite(l["final_loss"]) for l in legs.values() if "final_loss" in l)
    assert d["local_ms_per_step"] == legs["no process group (single-GPU step)"]["ms_per_step"]
    assert abs(d["scaling_efficiency"] - d["local_ms_per_step"] / d["ms_per_step"]) < 1e-3
    assert d["exposed_comm_ms"] is not None and d["exchange_path_overhead_ms"] is not None and d["fastest_dp_leg"]["ms_per_step"] > 0


def test_ungrouped_weight_gradient_option():
    """Default: one grouped weight-gradient GEMM per backward stage (stage hooks delayed by one stage).  B2S_DW_GROUP=0
    -- one split-K launch + slab reduce per weight gradient -- is the option: keep it correct too (fused trainer vs
    oracle and the 2-rank data-parallel run)."""
    import subprocess
    import sys
    if os.environ.get("B2S_DW_GROUP"):
        pytest.skip("inner run")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "tests/test_gpu_model.py", "tests/test_gpu_edge_dp.py",
                        "-k", "bf16 or two_ranks or fused_trainer"], cwd=root, env=dict(os.environ, B2S_DW_GROUP="0"),
                       capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]


@pytest.mark.parametrize("B,S,T", [(32, 50, 250), (9, 158, 808)])
def test_training_step_at_packer_extreme_shapes(B, S, T):
    """the two extremes of the reference's batch packer at full model size (many short / few long
    utterances).  bf16 fused trainer vs the fp32-mode HIP path on the same weights and batch: the loss terms agree
    within bf16 drift and three steps stay finite (the fp32 path itself is pinned to the oracle in test_gpu_model.py)."""
    import hyperparams
    from transformer.tacotron import Tacotron, compute_loss
    from b2s_hip.trainer import HipTrainer
    hp = hyperparams.hparams
    cfg = make_config("")
    st = synth.synthetic_state(cfg, 3)
    nb = synth.synthetic_batch(cfg, B, S, T, seed=5, n_spk=1, n_lang=1)
    batch = _dev(nb)
    vals = {}
    for mode in ("fp32", "bf16"):
        hp.override_from_dict(hyperparams.DEFAULTS)
        hp.parse("compute_dtype=%s,transformer_dropout_rate=0.0,decoder_dropout_rate=0.0" % mode)
        m = Tacotron(hp)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in st.items()})
        m = m.to(DEV).train()
        if mode == "fp32":
            o = m(**batch)
            vals[mode] = [float(x) for x in (lambda d: (d["loss"], d["bef_loss"], d["aft_loss"], d["stop_loss"]))(
                compute_loss(m, batch["mel_targets"], batch["target_lengths"], o, hp))]
        else:
            tr = HipTrainer(m, hp)
            v = tr.train_step(batch)
            vals[mode] = [float(v[0]), float(v[1]), float(v[2]), float(v[5])]
            for _ in range(2):
                v = tr.train_step(batch)
            assert torch.isfinite(v).all()
        del m
    for a, b in zip(vals["fp32"], vals["bf16"]):
        assert abs(a - b) < 0.03 * abs(a) + 1e-3, vals
    hp.override_from_dict(hyperparams.DEFAULTS)


@pytest.mark.parametrize("compute_dtype", ["fp32", "bf16"])
def test_padded_query_tiles_skipped_is_result_neutral(compute_dtype):
    """B2S_DEC_PADDED_UNOBSERVED (the trainer's decoder forward): the attention kernels do not compute 64-row tiles of padded target rows.
    Outputs (masked by target_lengths), the guided-attention term and d(memory) must be bit-identical to the full computation, the
    weight gradients equal up to the summation order of their atomics."""
    from b2s_hip.engine import _i32
    over = TINY + ",guided_attention_weight=2.0,transformer_dropout_rate=0.1,decoder_dropout_rate=0.1"
    m, cfg, st, hp = _build(over, compute_dtype=compute_dtype)
    B, S, T = 4, 70, 200
    nb = synth.synthetic_batch(cfg, B=B, S=S, T=T, seed=5, in_lens=[70, 9, 64, 33], tgt_lens=[200, 64, 1, 130])
    b = _dev(nb)
    eng = m.engine()
    in32, tgt32 = _i32(b["input_lengths"]), _i32(b["target_lengths"])
    g = torch.Generator(device="cpu").manual_seed(3)
    mem = torch.randn(B, S, hp.decoder_hidden, generator=g).to(DEV)          # (memory width = decoder width)
    dm = torch.randn(B, T, hp.num_mels, generator=g).to(DEV)          # (gradients at padded rows are NOT zero on entry: the engine masks them)
    ds = torch.randn(B, T, generator=g).to(DEV)
    dg = torch.ones(1, device=DEV)
    res = []
    for flag in (False, True):
        mels, stop, c = eng.decoder_forward(mem, in32, b["mel_targets"], tgt32, True, 77, True, padded_unobserved=flag)
        gl = eng.guided_loss(c).clone()
        dmem = eng.decoder_backward(c, dm, ds, mem.shape, dg)
        torch.cuda.synchronize()
        grads = {n: eng.grad_view(n).clone() for n, _ in m.named_parameters() if n.startswith("decoder.")}
        res.append((mels.clone(), stop.clone(), gl, dmem.clone(), grads))
        eng._needs_zero = True
    a, bb = res
    for i in range(4):
        assert torch.equal(a[i], bb[i]), i
    for n in a[4]:            # (weight-gradient reductions use fp32 atomics: run-to-run order differs, so not bit-for-bit)
        d = float((a[4][n] - bb[4][n]).abs().max())
        assert d <= 2e-5 * max(1.0, float(a[4][n].abs().max())), (n, d)
    assert float(a[3].abs().max()) > 0
