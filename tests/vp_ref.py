"""NumPy restatement of libb2s_vp.so (include/b2s_vp.h, DESIGN.md section p): a variance predictor, forward and backward, stage by
stage.  Every fp32 operation is made on its own in the order of the definition, so the library's results are these bits.

fmaf does not exist in NumPy; fma32 gets it exactly: the product of two fp32 is exact in fp64 (48 bits), its sum with c goes through
an error-free TwoSum, the fp64 sum is rounded to odd when the error is not zero, and one rounding to fp32 follows.  53 >= 2 * 24 + 2
bits, so the rounding to odd keeps everything the final rounding needs and there is no double rounding.  Everything is vectorised over
rows and filters, so a chain of K steps is K array operations."""
import numpy as np

OK, EMPTY, FAILED = 0, 1, 2
MAX_S, MAX_D = 1024, 1024
FILTERS = (64, 128, 256, 512)
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def align256(v):
    return (v + 255) // 256 * 256


def ws_bytes(B, S, D, F):
    return 256 + 2 * align256(3 * D * F * 4) + 2 * align256(3 * F * F * 4) + 3 * align256(B * S * F * 4) + align256((5 * F + 1) * B * 4)


def tape_bytes(B, S, F):
    return 5 * align256(B * S * F * 4) + 2 * align256(B * S * 4)


def fma32(a, b, c):
    """fmaf(a, b, c) of fp32 arrays (broadcast), one rounding."""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)      # exact
    c = np.asarray(c, np.float32).astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                       # TwoSum: p + c == s + err exactly
    s, err = np.broadcast_arrays(s, err)
    w = s.copy().view(np.int64)
    need = (err != 0) & ((w & 1) == 0)                    # inexact and even: the neighbour towards the error is the odd one
    step = np.where((err > 0) == (s > 0), 1, -1)          # one ulp away from zero or towards it, in the sign-magnitude pattern
    w = np.where(need, w + step, w)
    return w.view(np.float64).astype(np.float32)


def tree(v):
    """v[..., F] -> [...]: halves added onto each other until one value is left."""
    v = np.asarray(v, np.float32)
    while v.shape[-1] > 1:
        h = v.shape[-1] // 2
        v = v[..., :h] + v[..., h:]
    return v[..., 0]


def lowbias32(x):
    x = np.asarray(x, np.uint64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def drop_constants(p, seed, site):
    """(key, thresh, scale) of the dropout at `site` (1 or 2)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lo, hi = seed & 0xFFFFFFFF, seed >> 32
    key = int(lowbias32((lo + 0x9E3779B9 * site) & 0xFFFFFFFF)) ^ int(lowbias32(hi ^ 0x85EBCA6B))
    return key, int(np.floor(float(p) * 4294967296.0)), np.float32(1.0 / (1.0 - float(p)))


def mask(p, seed, site, B, S, F):
    """keep [B, S, F] bool."""
    key, thresh, _ = drop_constants(p, seed, site)
    idx = np.arange(B * S * F, dtype=np.uint64) & 0xFFFFFFFF
    return (lowbias32((idx * 0x9E3779B1 + key) & 0xFFFFFFFF) >= thresh).reshape(B, S, F)


def statuses(n, S):
    n = np.asarray(n)
    return np.where((n < 0) | (n > S), FAILED, np.where(n == 0, EMPTY, OK)).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- the stages

def conv(inp, W, bias):
    """inp [n, C] (the valid rows of one utterance), W [F, C, 3], bias [F] -> a [n, F]."""
    n, C = inp.shape
    pad = np.zeros((n + 2, C), np.float32)
    pad[1:n + 1] = inp
    acc = np.broadcast_to(np.asarray(bias, np.float32)[None, :], (n, W.shape[0])).copy()
    for j in range(3):
        for c in range(C):
            acc = fma32(pad[j:j + n, c][:, None], W[None, :, c, j], acc)
    return acc


def norm(a, g, be, eps, keep, scale):
    """a [n, F] -> (xh, rstd [n], h): ReLU, LayerNorm, dropout (keep None: p == 0)."""
    Ff = F32(a.shape[-1])
    r = np.where(a > 0, a, F32(0.0)).astype(np.float32)
    mu = tree(r) / Ff
    d = r - mu[:, None]
    var = tree(d * d) / Ff
    rstd = F32(1.0) / np.sqrt(var + F32(eps))
    xh = d * rstd[:, None]
    nrm = (xh * g[None, :]) + be[None, :]
    h = nrm if keep is None else np.where(keep, nrm * F32(scale), F32(0.0)).astype(np.float32)
    return xh, rstd.astype(np.float32), h.astype(np.float32)


def linear(h2, wl, bl):
    return tree(h2 * wl[None, :]) + F32(bl)


def norm_backward(dh, a, xh, rstd, g, keep, scale):
    """-> (dn, da)."""
    Ff = F32(a.shape[-1])
    dn = dh if keep is None else np.where(keep, dh * F32(scale), F32(0.0)).astype(np.float32)
    dxh = dn * g[None, :]
    m1 = tree(dxh) / Ff
    m2 = tree(dxh * xh) / Ff
    dr = ((dxh - m1[:, None]) - (xh * m2[:, None])) * rstd[:, None]
    return dn, np.where(a > 0, dr, F32(0.0)).astype(np.float32)


def conv_input_backward(da, W):
    """da [n, F], W [F, C, 3] -> din [n, C]."""
    n, F = da.shape
    pad = np.zeros((n + 2, F), np.float32)
    pad[1:n + 1] = da
    acc = np.zeros((n, W.shape[1]), np.float32)
    for j in range(3):
        for f in range(F):
            acc = fma32(pad[2 - j:2 - j + n, f][:, None], W[None, f, :, j], acc)      # row s + 1 - j
    return acc


def conv_weight_backward(das, inps, F, C):
    """Lists over the OK utterances in ascending b of da [n, F] and in [n, C] -> (dW [F, C, 3], db [F]): one chain each."""
    dW, db = np.zeros((F, C, 3), np.float32), np.zeros(F, np.float32)
    for da, inp in zip(das, inps):
        n = da.shape[0]
        pad = np.zeros((n + 2, C), np.float32)
        pad[1:n + 1] = inp
        for s in range(n):
            for j in range(3):
                dW[:, :, j] = fma32(da[s][:, None], pad[s + j][None, :], dW[:, :, j])
            db = db + da[s]
    return dW, db


def chain_add(rows):
    acc = np.zeros(rows.shape[1:], np.float32)
    for r in rows:
        acc = acc + r
    return acc


def chain_fma(a, b):
    acc = np.zeros(b.shape[1:], np.float32)
    for i in range(b.shape[0]):
        acc = fma32(a[i], b[i], acc)
    return acc


# --------------------------------------------------------------------------------------------------------------- the two calls

def _params(P):
    return [np.ascontiguousarray(P[k], np.float32) for k in ("W1", "b1", "g1", "be1", "W2", "b2", "g2", "be2", "wl", "bl")]


def forward(x, n, P, eps, p=0.0, seed=0, sentinel=0.0, masks=None):
    """-> dict: pred [B, S] (the rows of a FAILED utterance hold `sentinel`), status [B], and per OK utterance the stages that
    backward reads (`tape`: b -> dict).  masks: (keep1, keep2) [B, S, F] with p giving the scale, instead of the rule."""
    W1, b1, g1, be1, W2, b2, g2, be2, wl, bl = _params(P)
    B, S, _ = x.shape
    F = W1.shape[0]
    st = statuses(n, S)
    pred = np.zeros((B, S), np.float32)
    keep = [None, None]
    scale = F32(1.0)
    if p != 0.0:
        keep = list(masks) if masks is not None else [mask(p, seed, 1, B, S, F), mask(p, seed, 2, B, S, F)]
        scale = drop_constants(p, seed, 1)[2]
    tape = {}
    for b in range(B):
        if st[b] == FAILED:
            pred[b] = sentinel
        if st[b] != OK:
            continue
        nb = int(n[b])
        k1, k2 = (None if k is None else k[b, :nb] for k in keep)
        a1 = conv(x[b, :nb], W1, b1)
        xh1, rstd1, h1 = norm(a1, g1, be1, eps, k1, scale)
        a2 = conv(h1, W2, b2)
        xh2, rstd2, h2 = norm(a2, g2, be2, eps, k2, scale)
        pred[b, :nb] = linear(h2, wl, bl[0])
        tape[b] = {"a1": a1, "xh1": xh1, "rstd1": rstd1, "h1": h1, "a2": a2, "xh2": xh2, "rstd2": rstd2, "h2": h2, "k1": k1, "k2": k2}
    return {"pred": pred, "status": st, "tape": tape, "scale": scale}


def backward(x, n, P, fwd, d_pred):
    """The gradients of d_pred [B, S] through forward's result `fwd` -> dict dx, dW1, .., dbl."""
    W1, b1, g1, be1, W2, b2, g2, be2, wl, bl = _params(P)
    B, S, D = x.shape
    F = W1.shape[0]
    scale = fwd["scale"]
    dx = np.zeros((B, S, D), np.float32)
    das1, das2, xs, h1s = [], [], [], []
    parts = {k: [] for k in ("dbe2", "dg2", "dwl", "dbe1", "dg1", "dbl")}
    for b in sorted(fwd["tape"]):
        t = fwd["tape"][b]
        nb = int(n[b])
        dp = np.ascontiguousarray(d_pred[b, :nb], np.float32)
        dh2 = dp[:, None] * wl[None, :]
        dn2, da2 = norm_backward(dh2, t["a2"], t["xh2"], t["rstd2"], g2, t["k2"], scale)
        dh1 = conv_input_backward(da2, W2)
        dn1, da1 = norm_backward(dh1, t["a1"], t["xh1"], t["rstd1"], g1, t["k1"], scale)
        dx[b, :nb] = conv_input_backward(da1, W1)
        das1.append(da1), das2.append(da2), xs.append(x[b, :nb]), h1s.append(t["h1"])
        parts["dbe2"].append(chain_add(dn2)), parts["dg2"].append(chain_fma(dn2, t["xh2"]))
        parts["dwl"].append(chain_fma(dp[:, None], t["h2"])), parts["dbl"].append(chain_add(dp))
        parts["dbe1"].append(chain_add(dn1)), parts["dg1"].append(chain_fma(dn1, t["xh1"]))
    out = {"dx": dx}
    out["dW1"], out["db1"] = conv_weight_backward(das1, xs, F, D)
    out["dW2"], out["db2"] = conv_weight_backward(das2, h1s, F, F)
    for k, v in parts.items():
        shape = (1,) if k == "dbl" else (F,)
        out[k] = chain_add(np.asarray(v, np.float32).reshape((len(v),) + shape)) if v else np.zeros(shape, np.float32)
    return out


def durations_from_prediction(pred, n, alpha, max_frames):
    pred = np.asarray(pred, np.float64)
    d = np.clip(np.rint((np.exp(pred) - 1.0) * float(alpha)), 0, max_frames).astype(np.int32)
    d[np.arange(pred.shape[1])[None, :] >= np.asarray(n).reshape(-1, 1)] = 0
    return d
