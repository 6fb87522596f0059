"""Full-batch Lloyd k-means on the MI355X — the on-device way to thin a reference bank to `n_clusters` representatives.

The reference thins its dictionary with sklearn's MiniBatchKMeans on the host (/root/reference/dataloader_ref_cluster.py:106-144);
`ReferenceIndex.cluster_features()` keeps that estimator as its default so that its representatives are the reference's.  This module is
the opt-in alternative for banks that already live in HBM: plain Lloyd iterations (assign, then update) on the kernels of
csrc/kmeans.hip, deterministic bit for bit.  It is NOT the reference's estimator: the algorithm (full batch instead of mini-batch) and the
initialisation (sampled rows instead of k-means++) both differ, so the clusters differ too.

    kmeans_assign           nearest centre of every row: a blocked GEMM on the f32 matrix cores with a running (min, index) epilogue;
                            the [N, K] score matrix is never written
    kmeans_update           cluster means, members summed in ascending row order (512-row chunks for long lists)
    kmeans_representatives  per cluster the member closest to its centre (ties: lowest row), -1 for an empty cluster
    DeviceKMeans            sklearn-like estimator over the three
"""
from __future__ import annotations

import numpy as np
import torch

from . import lib as _lib
from .ops import _L, _stream


def _rows(t, what):
    """A [R, D] f32 GPU matrix the kernels can read in place: unit column stride, 16-byte aligned rows; anything else is copied."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.ClcError(f"{what}: GPU tensors only (no CPU fallback)")
    if t.dim() != 2:
        raise ValueError(f"{what}: expected a [rows, D] matrix, got shape {tuple(t.shape)}")
    t = t.float()
    ok = t.stride(1) == 1 and t.stride(0) >= t.shape[1] and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0
    return t if ok else t.contiguous()


def _check_shapes(N, D, K, what, k_le_n=True):
    if D < 4 or D % 4:
        raise ValueError(f"{what}: D={D} must be a multiple of 4 (>= 4)")
    if K < 1 or (k_le_n and K > N) or N < 1:
        raise ValueError(f"{what}: n_clusters={K} must be in 1..N={N}")


def _labels(labels, N, dev, what):
    if not torch.is_tensor(labels) or not labels.is_cuda:
        raise _lib.ClcError(f"{what}: GPU tensors only (no CPU fallback)")
    if labels.shape != (N,):
        raise ValueError(f"{what}: labels must have shape [{N}]")
    lab = labels.to(torch.int32).contiguous()
    # the inverted index: rows sorted by label, rows of one label ascending (stable)
    order = torch.argsort(lab, stable=True).to(torch.int32)
    return lab, order


def kmeans_assign(x, centres):
    """-> (labels int32 [N], score f32 [N]): labels[i] = argmin_k (|c_k|^2 - 2 x_i.c_k), equal scores -> lowest k; score = that minimum
    (squared distance = |x_i|^2 + score[i])."""
    x, c = _rows(x, "kmeans_assign"), _rows(centres, "kmeans_assign")
    (N, D), K = x.shape, c.shape[0]
    if c.shape[1] != D:
        raise ValueError("kmeans_assign: x and centres differ in D")
    _check_shapes(N, D, K, "kmeans_assign", k_le_n=False)            # assigning few rows to many centres is fine (predict)
    csq = (c.double() ** 2).sum(1).float()                       # |c|^2 in double, rounded once
    labels = torch.empty(N, device=x.device, dtype=torch.int32)
    score = torch.empty(N, device=x.device, dtype=torch.float32)
    _lib.check(_L().clc_kmeans_assign(x.data_ptr(), x.stride(0), N, D, c.data_ptr(), c.stride(0), K, csq.data_ptr(), labels.data_ptr(),
                                      score.data_ptr(), _stream()), "clc_kmeans_assign")
    return labels, score


def kmeans_update(x, labels, n_clusters, prev_centres):
    """-> (centres f32 [K, D], counts int32 [K]): the mean of each cluster's members (labels in [0, K)); an empty cluster keeps its row of
    prev_centres bit for bit."""
    x, p = _rows(x, "kmeans_update"), _rows(prev_centres, "kmeans_update")
    (N, D), K = x.shape, int(n_clusters)
    _check_shapes(N, D, K, "kmeans_update")
    if p.shape != (K, D):
        raise ValueError(f"kmeans_update: prev_centres must be [{K}, {D}]")
    lab, order = _labels(labels, N, x.device, "kmeans_update")
    out = torch.empty((K, D), device=x.device, dtype=torch.float32)
    counts = torch.empty(K, device=x.device, dtype=torch.int32)
    L = _L()
    nbytes = L.clc_kmeans_update_workspace_bytes(N, D, K)
    ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
    _lib.check(L.clc_kmeans_update(x.data_ptr(), x.stride(0), N, D, lab.data_ptr(), order.data_ptr(), K, p.data_ptr(), p.stride(0),
                                   out.data_ptr(), D, counts.data_ptr(), ws.data_ptr(), nbytes, _stream()), "clc_kmeans_update")
    return out, counts


def kmeans_representatives(x, labels, centres):
    """-> int64 [K]: per cluster the row index of the member with the smallest squared distance to its centre (ties: lowest row index),
    -1 for a cluster without members."""
    x, c = _rows(x, "kmeans_representatives"), _rows(centres, "kmeans_representatives")
    (N, D), K = x.shape, c.shape[0]
    if c.shape[1] != D:
        raise ValueError("kmeans_representatives: x and centres differ in D")
    _check_shapes(N, D, K, "kmeans_representatives")
    lab, order = _labels(labels, N, x.device, "kmeans_representatives")
    rep = torch.empty(K, device=x.device, dtype=torch.int32)
    L = _L()
    nbytes = L.clc_kmeans_representatives_workspace_bytes(K)
    ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
    _lib.check(L.clc_kmeans_representatives(x.data_ptr(), x.stride(0), N, D, lab.data_ptr(), order.data_ptr(), c.data_ptr(), c.stride(0), K,
                                            rep.data_ptr(), ws.data_ptr(), nbytes, _stream()), "clc_kmeans_representatives")
    return rep.long()


class DeviceKMeans:
    """Full-batch Lloyd k-means on the GPU with sklearn-like attributes (cluster_centers_, labels_, inertia_, n_iter_, counts_).

    An iteration is an assignment followed by an update.  fit() stops at the first assignment that changes no label (the centres are then
    the means of exactly these labels) or after `max_iter` updates, in which case one more assignment runs; either way labels_ equals
    predict(X) bit for bit.  n_iter_ counts the updates.  Empty clusters keep their previous centre (they are not relocated).
    init: "sample" draws K distinct rows with numpy's default_rng(seed) on the host, or pass a [K, D] array / tensor."""

    def __init__(self, n_clusters, max_iter=100, init="sample", seed=42):
        self.n_clusters, self.max_iter, self.init, self.seed = int(n_clusters), int(max_iter), init, int(seed)

    def _validated(self, X, fitting=True):
        if not torch.is_tensor(X) or not X.is_cuda:
            raise _lib.ClcError("DeviceKMeans: GPU tensors only (no CPU fallback)")
        if X.dim() != 2:
            raise ValueError(f"DeviceKMeans: expected [N, D], got shape {tuple(X.shape)}")
        _check_shapes(X.shape[0], X.shape[1], self.n_clusters, "DeviceKMeans", k_le_n=fitting)
        x = _rows(X, "DeviceKMeans")
        if not bool(torch.isfinite(x).all()):
            raise ValueError("DeviceKMeans: X holds non-finite values")
        return x

    def _init_centres(self, x):
        K, (N, D) = self.n_clusters, x.shape
        if isinstance(self.init, str):
            if self.init != "sample":
                raise ValueError(f"DeviceKMeans: init must be 'sample' or a [K, D] array, got {self.init!r}")
            rows = np.sort(np.random.default_rng(self.seed).choice(N, size=K, replace=False))
            return x[torch.as_tensor(rows, device=x.device)].contiguous()
        c = torch.as_tensor(np.asarray(self.init) if not torch.is_tensor(self.init) else self.init).to(device=x.device, dtype=torch.float32)
        if c.shape != (K, D):
            raise ValueError(f"DeviceKMeans: init must be [{K}, {D}], got {tuple(c.shape)}")
        if not bool(torch.isfinite(c).all()):
            raise ValueError("DeviceKMeans: init holds non-finite values")
        return c.contiguous().clone()

    @torch.no_grad()
    def fit(self, X):
        x = self._validated(X)
        c = self._init_centres(x)
        prev, n_iter = None, 0
        while True:
            labels, score = kmeans_assign(x, c)
            if prev is not None and not bool((labels != prev).any()):   # the one scalar read of the iteration
                break
            if n_iter == self.max_iter:
                break
            c, _ = kmeans_update(x, labels, self.n_clusters, c)
            prev, n_iter = labels, n_iter + 1
        self.cluster_centers_, self.labels_, self.n_iter_ = c, labels, n_iter
        self.counts_ = torch.bincount(labels.long(), minlength=self.n_clusters).to(torch.int32)   # sizes under labels_ (integers)
        self.inertia_ = float(((x.double() ** 2).sum(1) + score.double()).sum())
        return self

    @torch.no_grad()
    def predict(self, X):
        return kmeans_assign(self._validated(X, fitting=False), self.cluster_centers_)[0]

    def fit_predict(self, X):
        return self.fit(X).labels_
