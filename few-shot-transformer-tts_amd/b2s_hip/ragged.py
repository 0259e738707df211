"""Ragged batches as the satellite libraries take them: packed rows with B + 1 int32 offsets.  Shared by metrics, mcd, f0, durations,
cer, vocoder and alignment."""
import numpy as np
import torch

from .cbind import B2SError


def device(subject, *arrays):
    """Where a call runs: the device of the first CUDA tensor among `arrays`, else the current HIP device.  `subject` opens the
    refusal when there is none ("the DTW metric", "the edit distance")."""
    for a in arrays:
        if isinstance(a, torch.Tensor) and a.is_cuda:
            return a.device
    if not torch.cuda.is_available():
        raise B2SError("%s runs on the GPU only; no HIP device is visible" % subject)
    return torch.device("cuda", torch.cuda.current_device())


def offsets(lengths, device=None):
    """B lengths -> their B + 1 int32 offsets as a host array; with `device`, (host array, its copy on the device)."""
    off = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(np.asarray(lengths, dtype=np.int64).reshape(-1), out=off[1:])
    if off[-1] >= 2 ** 31:
        raise B2SError("%d symbols in one batch: the offsets are int32" % off[-1])
    off = off.astype(np.int32)
    return off if device is None else (off, torch.from_numpy(off).to(device))


def lengths(lengths, B, T, what):
    """B lengths (list, array or tensor) as Python ints, each cut to T; a wrong count or a negative length is refused."""
    if isinstance(lengths, torch.Tensor):
        lengths = lengths.detach().cpu().numpy()
    out = [int(n) for n in np.asarray(lengths).reshape(-1)]
    if len(out) != B:
        raise B2SError("%d %s for a batch of %d" % (len(out), what, B))
    if any(n < 0 for n in out):
        raise B2SError("%s must be >= 0 (got %s)" % (what, out))
    return [min(n, T) for n in out]                    # x[i, :n] slices past the end like the reference's indexing


def as_tensor(a):
    """Array, list or tensor -> tensor where it is: a tensor detached, anything else through np.asarray without a copy."""
    return a.detach() if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))


def lengths_i32(lengths, B, device, what):
    """B lengths (list, array or tensor on any device) -> contiguous int32 tensor on `device`.  A wrong count is refused; nothing is
    clamped (the library clamps, or reports a length outside its range as FAILED) and a float is cut towards zero."""
    t = as_tensor(lengths).reshape(-1)
    if t.numel() != B:
        raise B2SError("%d %s for a batch of %d" % (t.numel(), what, B))
    return t.to(device=device, dtype=torch.int32, non_blocking=True).contiguous()


def as_batch(a, device, what):
    """[B, T, dim] (or [B, T] for dim 1) NumPy array or tensor on any device -> contiguous fp32 tensor [B, T, dim] on `device`."""
    t = as_tensor(a)
    if t.dim() == 2:
        t = t.unsqueeze(-1)
    if t.dim() != 3:
        raise B2SError("%s must be [B, T, dim] or [B, T], got %s" % (what, tuple(t.shape)))
    return t.to(device=device, dtype=torch.float32).contiguous()


def pack(t, lengths):
    """Padded [B, T, dim] -> packed [sum(lengths), dim] rows and their B + 1 int32 host offsets."""
    mask = torch.arange(int(t.shape[1])).unsqueeze(0) < torch.tensor(lengths, dtype=torch.int64).unsqueeze(1)
    return t[mask.to(t.device)].contiguous(), offsets(lengths)


def paths(out):
    """Host copies of the paths of a DTW result (path, path_len, host path_offsets): list of int64 [L_b, 2] arrays (empty for EMPTY
    / FAILED pairs)."""
    path = out["path"].cpu().numpy()
    plen = out["path_len"].cpu().numpy()
    po = out["path_offsets"]
    return [path[po[b]:po[b] + plen[b]].astype(np.int64) for b in range(len(plen))]
