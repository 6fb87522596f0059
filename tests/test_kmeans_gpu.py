"""On-device k-means (clc_amd/kmeans.py, csrc/kmeans.hip) against the float64 checker tests/kmeans_ref.py (pinned to sklearn by
tests/test_kmeans_cpu.py).  Every bound is derived, not measured:
  * two compared scores are off by at most tol_i = 2 (D + 2) 2^-24 (|x_i|^2 + max_k |c_k|^2) (kmeans_ref.tol);
  * a mean of n_k rows summed in f32 in any order is off by at most n_k 2^-24 max|x| per element."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_ref as ref  # noqa: E402

from clc_amd import kmeans as km  # noqa: E402  (fails on a tree without the feature)
from clc_amd.lib import ClcError  # noqa: E402

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _strided(x, pad=12, lead=4):
    """the same values behind a leading dimension of D + pad (rows stay 16-byte aligned)"""
    big = torch.zeros((x.shape[0], x.shape[1] + pad), device=x.device, dtype=x.dtype)
    v = big[:, lead:lead + x.shape[1]]
    v.copy_(x)
    assert v.stride(0) == x.shape[1] + pad
    return v


def _mean_bound(X, counts):
    return np.maximum(counts, 1)[:, None] * ref.U * np.abs(X).max()


# ---- 1. assignment against float64
@pytest.mark.parametrize("N,K,D", ref.ASSIGN_SHAPES)
def test_assign_matches_float64(dev, N, K, D):
    X, C = ref.assign_case(N, K, D)
    x, c = _t(X, dev), _t(C, dev)
    labels, score = km.kmeans_assign(x, c)
    assert labels.dtype == torch.int32 and score.dtype == torch.float32 and labels.shape == (N,) and score.shape == (N,)
    lab, sc = labels.cpu().numpy().astype(np.int64), score.cpu().numpy().astype(np.float64)
    assert lab.min() >= 0 and lab.max() < K
    d, t = ref.sqdist(X, C), ref.tol(X, C)
    dmin, chosen = d.min(1), d[np.arange(N), lab]
    near = ref.near_tied(d, t)
    excess = (chosen - dmin) / t
    serr = np.abs(sc - (dmin - (X.astype(np.float64) ** 2).sum(1))) / t
    print(f"({N}, {K}, {D}): excess/tol max {excess.max():.3g}, near-tied {near.mean():.3%}, label mismatches {(lab != d.argmin(1)).sum()}, "
          f"score err/tol max {serr.max():.3g}")
    assert (excess <= 1.0).all(), "a chosen centre is farther than the float64 minimum by more than tol_i"
    assert near.mean() <= 0.01
    assert np.array_equal(lab[~near], d.argmin(1)[~near])
    assert (serr <= 1.0).all()
    l2, s2 = km.kmeans_assign(_strided(x), c)
    assert torch.equal(l2, labels) and torch.equal(s2, score), "a leading dimension > D changed the bits"


# ---- 2. ties and exactness
def test_assign_integer_ties_go_to_the_lowest_index(dev):
    X, C, rows = ref.integer_ties()
    labels, score = km.kmeans_assign(_t(X, dev), _t(C, dev))
    lab = labels.cpu().numpy()
    d = ref.sqdist(X, C)
    assert np.array_equal(lab, d.argmin(1)), f"{(lab != d.argmin(1)).sum()} labels differ from the first-occurrence argmin"
    assert not np.isin(lab, [17, 100, 129]).any()
    assert (lab[rows["on5"]] == 5).all() and (lab[rows["on3"]] == 3).all() and (lab[rows["on7"]] == 7).all() and (lab[rows["mid"]] == 40).all()
    assert np.array_equal(score.cpu().numpy().astype(np.float64), d.min(1) - (X.astype(np.float64) ** 2).sum(1)), "integer scores are exact"


# ---- 3. update against float64
@pytest.mark.parametrize("N,K,D", [(3000, 37, 36), (700, 5, 2048)])
def test_update_matches_float64_means(dev, N, K, D):
    rng = np.random.default_rng(7 * N + D)
    X = rng.normal(size=(N, D)).astype(np.float32)
    prev = rng.normal(size=(K, D)).astype(np.float32)
    lab = rng.integers(0, K - 1, size=N)          # cluster K - 1 stays empty
    lab[lab == 2] = 3                             # and so does cluster 2
    x, p, l = _t(X, dev), _t(prev, dev), _t(lab.astype(np.int32), dev)
    cen, counts = km.kmeans_update(x, l, K, p)
    want, wcounts = ref.means(X, lab, K, prev)
    assert counts.dtype == torch.int32 and np.array_equal(counts.cpu().numpy(), wcounts)
    got = cen.cpu().numpy()
    err = np.abs(got.astype(np.float64) - want) / _mean_bound(X, wcounts)
    print(f"({N}, {K}, {D}): mean err / bound max {err.max():.3g}")
    assert (err <= 1.0).all()
    for k in (2, K - 1):
        assert wcounts[k] == 0 and np.array_equal(got[k].view(np.uint32), prev[k].view(np.uint32)), "an empty cluster must keep its centre bit for bit"
    cen2, counts2 = km.kmeans_update(x, l, K, p)
    assert torch.equal(cen2, cen) and torch.equal(counts2, counts), "a second call gave other bits"
    cen3, _ = km.kmeans_update(_strided(x), l.long(), K, p)
    assert torch.equal(cen3, cen), "a leading dimension > D (or int64 labels) changed the bits"


def test_update_one_long_list(dev):
    """all 3000 points in one of three clusters: the member list is cut into six 512-row chunks"""
    rng = np.random.default_rng(3)
    X = (rng.normal(size=(3000, 36)) + 3.0).astype(np.float32)
    prev = rng.normal(size=(3, 36)).astype(np.float32)
    lab = np.full(3000, 1, np.int32)
    cen, counts = km.kmeans_update(_t(X, dev), _t(lab, dev), 3, _t(prev, dev))
    want, wcounts = ref.means(X, lab, 3, prev)
    got = cen.cpu().numpy()
    assert counts.cpu().tolist() == [0, 3000, 0]
    assert (np.abs(got[1].astype(np.float64) - want[1]) <= 3000 * ref.U * np.abs(X).max()).all()
    assert np.array_equal(got[[0, 2]].view(np.uint32), prev[[0, 2]].view(np.uint32))
    cen2, _ = km.kmeans_update(_t(X, dev), _t(lab, dev), 3, _t(prev, dev))
    assert torch.equal(cen2, cen)


def test_update_several_long_lists_among_short_and_empty_ones(dev):
    """cluster sizes 1300, 0, 600, 1, 1099 (rows interleaved): 3 + 0 + 2 + 1 + 3 chunk slots, so the chunk -> cluster search and the
    chunk-order sum of the partials see multi-chunk lists next to a one-row list and an empty one"""
    sizes = [1300, 0, 600, 1, 1099]
    rng = np.random.default_rng(11)
    X = (rng.normal(size=(3000, 36)) + 3.0).astype(np.float32)
    prev = rng.normal(size=(5, 36)).astype(np.float32)
    lab = rng.permutation(np.repeat(np.arange(5), sizes)).astype(np.int32)
    cen, counts = km.kmeans_update(_t(X, dev), _t(lab, dev), 5, _t(prev, dev))
    want, wcounts = ref.means(X, lab, 5, prev)
    got = cen.cpu().numpy()
    assert counts.cpu().tolist() == sizes == wcounts.tolist()
    err = np.abs(got.astype(np.float64) - want) / _mean_bound(X, wcounts)
    print(f"sizes {sizes}: mean err / bound max {err.max():.3g}")
    assert (err <= 1.0).all()
    assert np.array_equal(got[1].view(np.uint32), prev[1].view(np.uint32)), "the empty cluster must keep its centre bit for bit"
    only = int(np.where(lab == 3)[0][0])
    assert np.array_equal(got[3].view(np.uint32), X[only].view(np.uint32)), "a one-member cluster's mean is that row"
    cen2, _ = km.kmeans_update(_t(X, dev), _t(lab, dev), 5, _t(prev, dev))
    assert torch.equal(cen2, cen)


# ---- 4. Lloyd steps are valid, and fit is the loop
def test_lloyd_steps_never_raise_the_objective_and_fit_is_the_loop(dev):
    X, C0 = ref.overlap()
    x, c = _t(X, dev), _t(C0, dev)
    K, max_iter = len(C0), 100
    prev, n_iter, obj = None, 0, None
    while True:
        labels, _ = km.kmeans_assign(x, c)
        lab, Cn = labels.cpu().numpy().astype(np.int64), c.cpu().numpy()
        slack = float(ref.tol(X, Cn).sum())
        now = ref.objective(X, Cn, lab)
        assert obj is None or now <= obj + slack, f"assignment {n_iter} raised the objective: {obj} -> {now} (slack {slack})"
        obj = now
        if prev is not None and not bool((labels != prev).any()):
            break
        if n_iter == max_iter:
            break
        c, _ = km.kmeans_update(x, labels, K, c)
        now = ref.objective(X, c.cpu().numpy(), lab)
        assert now <= obj + slack, f"update {n_iter} raised the objective: {obj} -> {now}"
        obj, prev, n_iter = now, labels, n_iter + 1
    assert 5 <= n_iter < max_iter, n_iter
    est = km.DeviceKMeans(K, max_iter=max_iter, init=C0).fit(x)
    assert est.n_iter_ == n_iter and torch.equal(est.labels_, labels) and torch.equal(est.cluster_centers_, c), "fit is not the hand-written loop"
    assert torch.equal(est.predict(x), est.labels_)
    assert np.array_equal(est.counts_.cpu().numpy(), np.bincount(lab, minlength=K))
    assert abs(est.inertia_ - obj) <= slack + 1e-6 * obj
    again = km.DeviceKMeans(K, max_iter=max_iter, init=_t(C0, dev)).fit(x)
    assert again.n_iter_ == n_iter and torch.equal(again.labels_, est.labels_) and torch.equal(again.cluster_centers_, est.cluster_centers_)
    capped = km.DeviceKMeans(K, max_iter=2, init=C0).fit(x)
    assert capped.n_iter_ == 2 and torch.equal(capped.predict(x), capped.labels_), "labels_ must be predict(X) at max_iter too"


# ---- 5. blobs end to end
def test_blobs_end_to_end(dev):
    X, C0 = ref.blobs()
    r = ref.lloyd(X, C0)
    x = _t(X, dev)
    est = km.DeviceKMeans(16, init=C0).fit(x)
    assert np.array_equal(est.labels_.cpu().numpy(), r["labels"]), "well-separated blobs: every label must be the float64 Lloyd's"
    counts = np.bincount(r["labels"], minlength=16)
    assert (np.abs(est.cluster_centers_.cpu().numpy().astype(np.float64) - r["centres"]) <= _mean_bound(X, counts)).all()
    assert est.n_iter_ == r["n_iter"] and est.fit_predict(x) is est.labels_
    a, b = km.DeviceKMeans(16, init="sample", seed=5).fit(x), km.DeviceKMeans(16, init="sample", seed=5).fit(x)
    assert torch.equal(a.cluster_centers_, b.cluster_centers_) and torch.equal(a.labels_, b.labels_) and a.n_iter_ == b.n_iter_ and a.inertia_ == b.inertia_


# ---- 6. representatives
def test_representatives_match_the_host_rule(dev):
    from clc_amd.retrieval import ReferenceIndex

    X, C0, _ = ref.integer_ties()
    K = len(C0)
    lab = ref.sqdist(X, C0).argmin(1)
    cen, counts = ref.means(X, lab, K, C0)
    cen = cen.astype(np.float32)
    assert (counts[[17, 100, 129]] == 0).all()
    d, t = ref.sqdist(X, cen)[np.arange(len(X)), lab], ref.tol(X, cen)
    want = np.full(K, -1, np.int64)
    for k in range(K):
        members = np.where(lab == k)[0]
        if len(members) == 0:
            continue
        j = members[np.argmin(d[members])]                 # the first minimum among the members
        want[k] = j
        close = members[d[members] <= d[j] + t[members]]
        # precondition on the float64 side, so that an f32 evaluation has one right answer: whoever comes within tolerance of the winner
        # either IS the winner's row (same bits -> same f32 distance -> the first one wins under any arithmetic), or the centre is a
        # multiple of 1/4 (clusters of 1, 2 or 4 integer rows: a pair is always equidistant from its mean), where every f32 product and
        # sum is exact (|x - c|^2 terms are multiples of 1/16 below 2^12) and an exact tie goes to the first row in f32 as in float64
        quarter = np.array_equal(4.0 * cen[k], np.round(4.0 * cen[k]))
        assert (X[close] == X[j]).all() or quarter, f"cluster {k}: distinct members within tolerance of the minimum"
    rep = km.kmeans_representatives(_t(X, dev), _t(lab.astype(np.int32), dev), _t(cen, dev))
    assert rep.dtype == torch.int64 and np.array_equal(rep.cpu().numpy(), want)
    assert (want[[17, 100, 129]] == -1).all()
    ix = ReferenceIndex(X, None, device=dev)
    ix.cluster_features(K, labels=lab, centers=cen)
    assert ix.representatives == [int(j) for j in want if j >= 0], "the index skips empty clusters and keeps cluster order"


# ---- 7. through the index
def test_device_method_through_the_index(dev):
    from sklearn.cluster import MiniBatchKMeans
    from sklearn.neighbors import NearestNeighbors

    from clc_amd.retrieval import ReferenceIndex

    rng = np.random.default_rng(5)
    bank = rng.normal(size=(3000, 256)).astype(np.float32)
    keys = {i: f"k{i}" for i in range(len(bank))}
    ix = ReferenceIndex(bank, keys, n_clusters=40, n_refs=2, device=dev, cluster_method="device")
    reps, labels = ix.representatives, ix.kmeans_.labels_.cpu().numpy()
    nonempty = [k for k in range(40) if (labels == k).any()]
    assert len(reps) == len(nonempty) and len(set(reps)) == len(reps)
    assert [int(labels[j]) for j in reps] == nonempty, "every representative is a member of its own cluster, in cluster order"
    assert ix.feature_to_key == {n: keys[j] for n, j in enumerate(reps)}
    assert ix.ref_features.shape == (len(reps), 256) and np.array_equal(ix.ref_features.cpu().numpy(), bank[reps])
    q = rng.normal(size=(9, 256)).astype(np.float32)
    _, idx_ref = NearestNeighbors(n_neighbors=2, algorithm="ball_tree").fit(bank[reps]).kneighbors(q)
    assert np.array_equal(ix.kneighbors(q)[1].cpu().numpy(), idx_ref)
    # the same through cluster_features(method="device") on a plain index: deterministic
    ix_b = ReferenceIndex(bank, keys, n_refs=2, device=dev)
    ix_b.cluster_features(40, method="device")
    assert ix_b.representatives == reps
    # the default construction is still the reference's estimator
    skm = MiniBatchKMeans(n_clusters=40, random_state=42, batch_size=1000)
    sl = skm.fit_predict(bank)
    want = []
    for i in range(40):
        members = np.where(sl == i)[0]
        if len(members):
            want.append(int(members[np.argmin(np.linalg.norm(bank[members] - skm.cluster_centers_[i], axis=1))]))
    assert ReferenceIndex(bank, keys, n_clusters=40, n_refs=2, device=dev).representatives == want


# ---- 8. argument errors
def test_argument_errors(dev):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(64, 8, generator=g).to(dev)
    with pytest.raises(ValueError):
        km.DeviceKMeans(4).fit(torch.randn(64, 6, generator=g).to(dev))      # D = 6
    with pytest.raises(ValueError):
        km.DeviceKMeans(65).fit(x)                                            # K > N
    with pytest.raises(ValueError):
        km.DeviceKMeans(0).fit(x)                                             # K = 0
    bad = x.clone()
    bad[3, 1] = float("nan")
    with pytest.raises(ValueError):
        km.DeviceKMeans(4).fit(bad)                                           # a NaN in X
    with pytest.raises(ClcError):
        km.DeviceKMeans(4).fit(x.cpu())                                       # a CPU tensor
    with pytest.raises(ClcError):
        km.kmeans_assign(x.cpu(), x[:4])
    with pytest.raises(ClcError):
        km.kmeans_update(x, torch.zeros(64, dtype=torch.int32), 4, x[:4])
    with pytest.raises(ClcError):
        km.kmeans_representatives(x, torch.zeros(64, dtype=torch.int32, device=dev), x[:4].cpu())
    with pytest.raises(ValueError):
        km.kmeans_assign(x[:, :6], x[:4, :6])
    with pytest.raises(ValueError):
        km.kmeans_update(x, torch.zeros(64, dtype=torch.int32, device=dev), 65, x)
