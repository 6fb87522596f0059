"""Float64 references of the patch-matching operations (clc_amd/patch_matching.py, csrc/patch_match.hip), written from the
definitions instead of from the kernels: the Pearson map by centring both sides, the normalisation + colour transform, the ordering
rule of the top-k search and the weighted patch gather.  The reference of tests/test_patch_matching_ref_cpu.py (which pins this
module to the golden file and to torch) and of tests/test_patch_matching_kernels_gpu.py.

THE ORDERING RULE (``topk``), torch.topk / torch.argmax's: NaN ranks above +inf, +inf above every finite value; equal entries take
the lowest index first, and all NaNs count as equal.
"""
import numpy as np
import torch
import torch.nn.functional as F

MEANS = (93.70454143384742, 98.28243432206516, 94.84678088809876)
VARS = (73.56493292844912, 75.88547006820752, 76.74838442810665)


def pearson_map(q, y):
    """q: patches [P,C,ph,pw]; y: image [1,C,H,W] -> [1,P,H-ph+1,W-pw+1] float64, the Pearson correlation of every patch with every
    window: both sides centred, xc yc^T / sqrt(sum xc^2 (x) sum yc^2)."""
    q, y = q.double(), y.double()
    P, C, ph, pw = q.shape
    H, W = y.shape[2], y.shape[3]
    win = F.unfold(y, (ph, pw))[0].t()                     # [npos, K], K in (c, dy, dx) order like q.reshape(P, -1)
    xc = q.reshape(P, -1)
    xc = xc - xc.mean(1, keepdim=True)
    yc = win - win.mean(1, keepdim=True)
    den = torch.sqrt((xc * xc).sum(1)[:, None] * (yc * yc).sum(1)[None, :])
    return ((xc @ yc.t()) / den).reshape(1, P, H - ph + 1, W - pw + 1)


def prep(x, in_scale):
    """rgb_transform(reduce_mean_and_std_normalize_images(x * in_scale)) in float64: [N,3,H,W] -> [N,3,H,W]."""
    x = x.double() * float(in_scale)
    R, G, B = ((x[:, c] - MEANS[c]) / VARS[c] for c in range(3))
    return torch.stack([R + G, R - G, 0.5 * (R + B)], dim=1)


def topk(row, k):
    """The k first entries of ``row`` ([n], or [P, n] row by row) under the ordering rule -> (values, indices int64), numpy."""
    a = np.asarray(row.detach().cpu().numpy() if torch.is_tensor(row) else row)
    if a.ndim == 2:
        vs, ix = zip(*(topk(r, k) for r in a))
        return np.stack(vs), np.stack(ix)
    assert a.ndim == 1 and 1 <= k <= a.shape[0]
    nan = np.isnan(a)
    desc = np.where(nan, 0.0, -a.astype(np.float64))       # descending values (-(+inf) first); the NaNs all equal
    order = np.lexsort((np.arange(a.shape[0]), desc, ~nan))[:k]   # keys, last one first: NaN, value, index
    return a[order], order.astype(np.int64)


def gather(y, idx, val, k, temperature, ph, pw):
    """y [1,C,H,W] (or [C,H,W]); idx [P,k] flat positions in the (H-ph+1) x (W-pw+1) map, P = (H/ph)(W/pw) query patches in row-major
    tiling order; val [P,k] -> [1,C,H,W] float64.  temperature < 0: candidate 0 copied as it is; else the softmax(val * temperature)
    weighted sum of the k candidates."""
    y = y.double().reshape((-1,) + tuple(y.shape[-2:]))
    C, H, W = y.shape
    cw = W - pw + 1
    idx = torch.as_tensor(np.asarray(idx)).long().reshape(-1, k)
    assert idx.shape[0] == (H // ph) * (W // pw) and int(idx.min()) >= 0 and int(idx.max()) < (H - ph + 1) * cw
    if temperature < 0:
        wgt = torch.zeros(idx.shape, dtype=torch.float64)
        wgt[:, 0] = 1.0
    else:
        wgt = torch.softmax(torch.as_tensor(np.asarray(val)).double().reshape(-1, k) * float(temperature), dim=1)
    out = torch.zeros(1, C, H, W, dtype=torch.float64)
    bw = W // pw
    for n in range(idx.shape[0]):
        by, bx = n // bw, n % bw
        acc = torch.zeros(C, ph, pw, dtype=torch.float64)
        for j in range(k if temperature >= 0 else 1):
            iy, ix = int(idx[n, j]) // cw, int(idx[n, j]) % cw
            acc += wgt[n, j] * y[:, iy:iy + ph, ix:ix + pw]
        out[0, :, by * ph:(by + 1) * ph, bx * pw:(bx + 1) * pw] = acc
    return out
