"""fp64 NumPy / SciPy restatement of fastdtw 0.3.4 (fastdtw(x, y, radius, dist=scipy.spatial.distance.euclidean) and
dtw(x, y)) in the library's literal dict and set form, plus the reference's calculate_mse_dtw on top of it -- the oracle of
tests/test_dtw_host.py and tests/test_gpu_dtw.py, written from the specification in DESIGN.md section h.

Indices are 0-based; D is 1-based with D[0, 0] = 0 and every cell outside the window +inf.  Each window cell takes
min((D[i-1, j] + dt, up), (D[i, j-1] + dt, left), (D[i-1, j-1] + dt, diag)) by cost only, so ties keep the first (Python's min).
`window_intervals` is the one-interval-per-row form of `expand_window` that the GPU kernel uses."""
from collections import defaultdict

import numpy as np

try:
    from scipy.spatial.distance import euclidean
except ImportError:                      # scipy's euclidean is sqrt(dot(u - v, u - v)) on fp64 vectors
    def euclidean(u, v):
        d = np.asarray(u, dtype=np.float64) - np.asarray(v, dtype=np.float64)
        return float(np.sqrt(np.dot(d, d)))


def _prep(x):
    x = np.asanyarray(x, dtype="float")
    return x


def _dist(a, b):
    return euclidean(np.atleast_1d(a), np.atleast_1d(b))


def dtw_window(x, y, window, dist=_dist):
    """The library's __dtw: windowed DTW over the 0-based cells of `window` (row-major), or the full matrix for None."""
    len_x, len_y = len(x), len(y)
    if window is None:
        window = [(i, j) for i in range(len_x) for j in range(len_y)]
    D = defaultdict(lambda: (float("inf"),))
    D[0, 0] = (0, 0, 0)
    for i, j in ((i + 1, j + 1) for i, j in window):
        dt = dist(x[i - 1], y[j - 1])
        D[i, j] = min((D[i - 1, j][0] + dt, i - 1, j), (D[i, j - 1][0] + dt, i, j - 1),
                      (D[i - 1, j - 1][0] + dt, i - 1, j - 1), key=lambda a: a[0])
    path = []
    i, j = len_x, len_y
    while not (i == j == 0):
        path.append((i - 1, j - 1))
        i, j = D[i, j][1], D[i, j][2]
    path.reverse()
    return D[len_x, len_y][0], path


def dtw(x, y, dist=_dist):
    return dtw_window(_prep(x), _prep(y), None, dist)


def reduce_by_half(x):
    return [(x[i] + x[1 + i]) / 2 for i in range(0, len(x) - len(x) % 2, 2)]


def expand_window(path, len_x, len_y, radius):
    """The library's __expand_window, set form."""
    path_ = set(path)
    for i, j in path:
        for a, b in ((i + a, j + b) for a in range(-radius, radius + 1) for b in range(-radius, radius + 1)):
            path_.add((a, b))
    window_ = set()
    for i, j in path_:
        for a, b in ((i * 2, j * 2), (i * 2, j * 2 + 1), (i * 2 + 1, j * 2), (i * 2 + 1, j * 2 + 1)):
            window_.add((a, b))
    window = []
    start_j = 0
    for i in range(0, len_x):
        new_start_j = None
        for j in range(start_j, len_y):
            if (i, j) in window_:
                window.append((i, j))
                if new_start_j is None:
                    new_start_j = j
            elif new_start_j is not None:
                break
        start_j = new_start_j
    return window


def window_intervals(path, len_x, len_y, radius):
    """Interval form of expand_window: fine row i (c = i // 2) spans [max(0, 2 (min pj - r)), min(len_y - 1, 2 (max pj + r) + 1)]
    over the coarse path cells with |pi - c| <= r.  Returns (lo, hi) int arrays of length len_x."""
    path = np.asarray(path, dtype=np.int64)
    lo = np.empty(len_x, np.int64)
    hi = np.empty(len_x, np.int64)
    for i in range(len_x):
        near = path[np.abs(path[:, 0] - i // 2) <= radius]
        lo[i] = max(0, 2 * (int(near[:, 1].min()) - radius))
        hi[i] = min(len_y - 1, 2 * (int(near[:, 1].max()) + radius) + 1)
    return lo, hi


def intervals_to_window(lo, hi):
    return [(i, j) for i in range(len(lo)) for j in range(int(lo[i]), int(hi[i]) + 1)]


def _fastdtw(x, y, radius, dist):
    min_time_size = radius + 2
    if len(x) < min_time_size or len(y) < min_time_size:
        return dtw_window(x, y, None, dist)
    distance, path = _fastdtw(reduce_by_half(x), reduce_by_half(y), radius, dist)
    window = expand_window(path, len(x), len(y), radius)
    return dtw_window(x, y, window, dist)


def fastdtw(x, y, radius=1, dist=_dist):
    """fastdtw 0.3.4 for radius >= 1: (distance, path as a list of (i, j))."""
    if radius < 1:
        raise ValueError("radius must be >= 1")
    x, y = _prep(x), _prep(y)
    return _fastdtw(x, y, radius, dist)


def calculate_mse_dtw(preds, pred_lengths, targets, target_lengths, radius=1):
    """The reference's calculate_mse_dtw on NumPy arrays: voiced frames (max over the features > 0), fastdtw with euclidean
    distance, then np.square(x[pathx] - y[pathy]).mean() in the inputs' dtype; None where a side has no voiced frame."""
    results = []
    for i in range(len(preds)):
        x = preds[i, :pred_lengths[i]]
        y = targets[i, :target_lengths[i]]
        x = x[np.where(np.max(x, axis=-1) > 0)]
        y = y[np.where(np.max(y, axis=-1) > 0)]
        if len(x) == 0 or len(y) == 0:
            results.append(None)
            continue
        distance, path = fastdtw(x, y, radius=radius)
        pathx = [p[0] for p in path]
        pathy = [p[1] for p in path]
        results.append(np.square(x[pathx] - y[pathy]).mean())
    return results
