"""float64 checker of the on-device k-means (clc_amd/kmeans.py): plain Lloyd iterations in numpy, the tolerance the GPU tests use and the
test inputs they share with tests/test_kmeans_cpu.py, which pins this file against sklearn.

Rules (the ones of clc_amd.kmeans.DeviceKMeans): argmin takes the first occurrence, means are taken in float64, an empty cluster keeps
its centre, and the loop stops at the first assignment that changes no label or after `max_iter` updates.

Tolerance.  A dot product of length D in f32 is off by at most D 2^-24 |x||c| for any summation order, so two compared scores
|c|^2 - 2 x.c (the |c|^2 rounded once, the doubling exact) are off by at most
    tol_i = 2 (D + 2) 2^-24 (|x_i|^2 + max_k |c_k|^2).
A point whose best and second-best float64 distances differ by no more than tol_i is "near-tied"."""
import numpy as np

U = 2.0 ** -24


def sqdist(X, C):
    """float64 [N, K] squared distances (expanded form in float64: its own error is 1e-16 relative, nine orders below tol)."""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    return (X ** 2).sum(1)[:, None] - 2.0 * (X @ C.T) + (C ** 2).sum(1)[None, :]


def tol(X, C):
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    return 2.0 * (X.shape[1] + 2) * U * ((X ** 2).sum(1) + (C ** 2).sum(1).max())


def near_tied(d, t):
    """bool [N]: best and second-best distance within t (never with a single centre)."""
    if d.shape[1] < 2:
        return np.zeros(d.shape[0], bool)
    two = np.partition(d, 1, axis=1)[:, :2]
    return (two[:, 1] - two[:, 0]) <= t


def means(X, labels, K, prev):
    """float64 cluster means under `labels`; an empty cluster keeps its row of prev.  -> (centres [K, D], counts [K])"""
    X = np.asarray(X, np.float64)
    counts = np.bincount(labels, minlength=K)
    sums = np.zeros((K, X.shape[1]))
    np.add.at(sums, labels, X)
    out = np.array(prev, np.float64, copy=True)
    nz = counts > 0
    out[nz] = sums[nz] / counts[nz, None]
    return out, counts


def objective(X, C, labels):
    """sum_i |x_i - c_label(i)|^2 in float64, direct form"""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    return float(((X - C[labels]) ** 2).sum())


def lloyd(X, C0, max_iter=100):
    """-> dict(labels, centres, n_iter, inertia, near_share [per assignment], min_gap_over_tol, empty [any empty cluster ever])"""
    X = np.asarray(X, np.float64)
    C = np.array(C0, np.float64, copy=True)
    K = C.shape[0]
    prev, n_iter, share, ratio, empty = None, 0, [], np.inf, False
    while True:
        d = sqdist(X, C)
        labels = d.argmin(1)
        t = tol(X, C)
        share.append(float(near_tied(d, t).mean()))
        if K > 1:
            two = np.partition(d, 1, axis=1)[:, :2]
            ratio = min(ratio, float(((two[:, 1] - two[:, 0]) / t).min()))
        if prev is not None and np.array_equal(labels, prev):
            break
        if n_iter == max_iter:
            break
        C, counts = means(X, labels, K, C)
        empty |= bool((counts == 0).any())
        prev, n_iter = labels, n_iter + 1
    return dict(labels=labels, centres=C, n_iter=n_iter, inertia=objective(X, C, labels), near_share=share, min_gap_over_tol=ratio, empty=empty)


# ---- shared inputs (f32 values; the checker and sklearn see them widened to float64)
def blobs():
    """16 centres ~ 4 N(0, 1) in D = 36, 125 members each with sigma 0.5, rows shuffled; the start is one member per blob."""
    rng = np.random.default_rng(11)
    centres = 4.0 * rng.normal(size=(16, 36))
    X = (centres[:, None, :] + 0.5 * rng.normal(size=(16, 125, 36))).reshape(-1, 36)
    blob = np.repeat(np.arange(16), 125)
    perm = rng.permutation(len(X))
    X, blob = X[perm].astype(np.float32), blob[perm]
    C0 = np.stack([X[np.where(blob == b)[0][0]] for b in range(16)])
    return X, C0


def overlap():
    """N = 3000 standard-normal rows in D = 64, K = 50 sampled rows as the start."""
    rng = np.random.default_rng(12)
    X = rng.normal(size=(3000, 64)).astype(np.float32)
    C0 = X[np.sort(rng.choice(3000, size=50, replace=False))].copy()
    return X, C0


ASSIGN_SHAPES = [(1000, 33, 36), (257, 1, 4), (96, 64, 2048), (4099, 300, 256), (31, 40, 64)]


def assign_case(N, K, D):
    """Standard-normal rows and K centres = sampled rows + 0.25 noise (distinct rows while K <= N).
    The seed is fixed on the float64 side alone: the near-tied cap of the assignment test (1 % of the points) is a property of the input,
    and tests/test_kmeans_cpu.py asserts it without a device.  At (96, 64, 2048) that cap allows no near-tied point at all, while the 32
    rows that seed no centre have their two nearest centres within tol_i (about 1 against a spread of about 130) for roughly every other
    seed; N + K + D itself is such a seed (one point at 0.40 tol_i).  With this one the smallest gap there is 1.7 tol_i, and 7 of 4099
    points are near-tied at (4099, 300, 256)."""
    rng = np.random.default_rng(N + K + D + 2)
    X = rng.normal(size=(N, D)).astype(np.float32)
    C = (X[rng.permutation(N)[np.arange(K) % N]] + 0.25 * rng.normal(size=(K, D))).astype(np.float32)
    return X, C


def integer_ties():
    """Integers in [-8, 8], N = 1000, K = 130, D = 36: every f32 product and sum is exact.  Centre 17 copies centre 5; centre 100 copies
    centre 3 (another 32-centre MFMA tile and another wave's half of the 128-centre tile); centre 129 copies centre 7 (another 128-centre
    tile); centre 41 is centre 40 with +2 in coordinate 0.  20 points sit on each duplicated centre and 20 exactly midway between centres
    40 and 41, scattered over the rows."""
    rng = np.random.default_rng(13)
    C = rng.integers(-8, 9, size=(130, 36)).astype(np.float32)
    C[17], C[100], C[129] = C[5], C[3], C[7]
    C[40, 0] = min(C[40, 0], 6.0)
    C[41] = C[40]
    C[41, 0] += 2.0
    X = rng.integers(-8, 9, size=(1000, 36)).astype(np.float32)
    rows = rng.permutation(1000)[:80]
    X[rows[:20]], X[rows[20:40]], X[rows[40:60]] = C[5], C[3], C[7]
    mid = C[40].copy()
    mid[0] += 1.0
    X[rows[60:80]] = mid
    return X, C, dict(on5=rows[:20], on3=rows[20:40], on7=rows[40:60], mid=rows[60:80])
