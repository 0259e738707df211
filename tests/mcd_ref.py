"""fp64 NumPy restatement of mel-cepstral distortion after DTW (DESIGN.md section k) -- the oracle of tests/test_mcd_host.py and
tests/test_gpu_mcd.py, written from the definition, on top of the fastdtw restatement of tests/dtw_ref.py.

Per side: voiced frames (np.max over the bins > 0, which drops a frame holding a NaN), normalised mel -> natural-log magnitude with
every operation rounded on its own, c_k = sum_m ln_m D[k, m] accumulated from 0 in ascending m (the explicit loop: product and sum
are separate NumPy operations, so nothing is fused), rounded once to fp32.  Then fastdtw / dtw with euclidean distance on the fp32
cepstra and the mean over the path of db_scale * sqrt(2 * sum_k (cx_k - cy_k)^2) in fp64."""
import math
import types

import numpy as np

import dtw_ref

LN_SCALE = math.log(10.0) / 20.0
DB_SCALE = 10.0 / math.log(10.0)

HP = types.SimpleNamespace(max_abs_value=4.0, max_db=100, ref_db=20, symmetric_mel=True)


def dct_table(n_mels, order):
    k = np.arange(1, order + 1, dtype=np.float64)[:, None]
    m = np.arange(n_mels, dtype=np.float64)[None, :]
    return np.sqrt(2.0 / n_mels) * np.cos(np.pi / n_mels * (m + 0.5) * k)


def voiced(x):
    with np.errstate(invalid="ignore"):
        return np.where(np.max(x, axis=-1) > 0)[0]


def log_magnitude(x, hp=HP):
    a = np.asarray(x, dtype=np.float32).astype(np.float64)
    if hp.symmetric_mel:
        big = np.float64(hp.max_abs_value)
        a = (a + big) / (2.0 * big)
    a = np.clip(a, 0.0, 1.0)
    db = (a * np.float64(hp.max_db) - np.float64(hp.max_db)) + np.float64(hp.ref_db)
    return db * np.float64(LN_SCALE)


def cepstra(x, order=13, hp=HP, table=None):
    """[T, n_mels] normalised mel -> (fp32 cepstra of the voiced frames [n, order], indices of the voiced frames)."""
    x = np.asarray(x, dtype=np.float32)
    keep = voiced(x)
    ln = log_magnitude(x[keep], hp)
    D = dct_table(x.shape[1], order) if table is None else table
    acc = np.zeros((len(keep), order), np.float64)
    for m in range(x.shape[1]):
        acc = acc + ln[:, m, None] * D[None, :, m]
    return acc.astype(np.float32), keep


def path_distortion(cx, cy, path):
    """Per-step distortion in dB along the path, fp64 over the fp32 cepstra."""
    path = np.asarray(path, dtype=np.int64).reshape(-1, 2)
    e = cx[path[:, 0]].astype(np.float64) - cy[path[:, 1]].astype(np.float64)
    return DB_SCALE * np.sqrt(2.0 * np.sum(e * e, axis=1))


def mcd_dtw(x, y, order=13, radius=1, hp=HP):
    """One pair -> dict(mcd, dist, path, cx, cy), mcd None when a side has no voiced frame."""
    cx, _ = cepstra(x, order, hp)
    cy, _ = cepstra(y, order, hp)
    if len(cx) == 0 or len(cy) == 0:
        return {"mcd": None, "dist": np.zeros(0), "path": [], "cx": cx, "cy": cy}
    _, path = dtw_ref.dtw(cx, cy) if radius is None else dtw_ref.fastdtw(cx, cy, radius=radius)
    dist = path_distortion(cx, cy, path)
    return {"mcd": float(np.mean(dist)), "dist": dist, "path": path, "cx": cx, "cy": cy}


def calculate_mcd_dtw(preds, pred_lengths, targets, target_lengths, order=13, radius=1, hp=HP):
    return [mcd_dtw(preds[i][:pred_lengths[i]], targets[i][:target_lengths[i]], order, radius, hp)["mcd"]
            for i in range(len(preds))]
