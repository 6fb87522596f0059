"""Pins tests/kmeans_ref.py, the float64 checker the GPU tests of the on-device k-means lean on: its Lloyd loop gives sklearn's labels
(KMeans with a given start, one run, algorithm="lloyd", tol=0) on both shared inputs, and the inputs have the properties the GPU tests
assume — evaluated on the float64 side alone."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_ref as ref  # noqa: E402


@pytest.fixture(scope="module")
def runs():
    out = {}
    for name, make in (("blobs", ref.blobs), ("overlap", ref.overlap)):
        X, C0 = make()
        out[name] = (X, C0, ref.lloyd(X, C0))
    return out


@pytest.mark.parametrize("name", ["blobs", "overlap"])
def test_checker_matches_sklearn(runs, name):
    from sklearn.cluster import KMeans

    X, C0, r = runs[name]
    km = KMeans(n_clusters=len(C0), init=C0.astype(np.float64), n_init=1, algorithm="lloyd", tol=0, max_iter=300).fit(X.astype(np.float64))
    assert not r["empty"], "sklearn relocates empty clusters, the checker keeps them: the inputs must not produce one"
    assert np.array_equal(km.labels_, r["labels"]), f"{(km.labels_ != r['labels']).mean():.2%} of the labels differ"
    assert abs(km.inertia_ - r["inertia"]) <= 1e-6 * r["inertia"], (km.inertia_, r["inertia"])
    assert np.allclose(km.cluster_centers_, r["centres"], rtol=0, atol=1e-9)


def test_inputs_have_the_assumed_margins(runs):
    _, _, b = runs["blobs"]
    _, _, o = runs["overlap"]
    print(f"blobs: {b['n_iter']} iterations, min gap / tol {b['min_gap_over_tol']:.3g}; overlap: {o['n_iter']} iterations, "
          f"near-tied share max {max(o['near_share']):.3%}")
    assert max(b["near_share"]) == 0.0 and b["min_gap_over_tol"] > 100.0   # blobs: the GPU run must reproduce every label
    assert max(o["near_share"]) <= 0.01                                     # overlap: at most 1 % of the points near-tied, per iteration
    assert o["n_iter"] >= 5, "the overlap set is meant to take several iterations"


@pytest.mark.parametrize("N,K,D", ref.ASSIGN_SHAPES)
def test_assign_inputs_meet_the_near_tied_cap(N, K, D):
    X, C = ref.assign_case(N, K, D)
    d, t = ref.sqdist(X, C), ref.tol(X, C)
    near = ref.near_tied(d, t)
    gap = np.diff(np.partition(d, 1, axis=1)[:, :2], axis=1)[:, 0] / t if K > 1 else np.full(N, np.inf)
    print(f"({N}, {K}, {D}): near-tied {near.sum()} of {N}, smallest gap / tol {gap.min():.3g}, smallest above 1: {gap[gap > 1].min():.3g}")
    assert near.mean() <= 0.01
    # no gap sits so close to tol_i that another BLAS could move it across (float64 distances are good to 1e-12 relative)
    assert (np.abs(gap - 1.0) > 1e-6).all()
    assert len(np.unique(C, axis=0)) == K


def test_integer_ties_input():
    X, C, rows = ref.integer_ties()
    assert np.abs(X).max() <= 8 and np.abs(C).max() <= 8 and np.array_equal(X, np.round(X)) and np.array_equal(C, np.round(C))
    assert np.array_equal(C[17], C[5]) and np.array_equal(C[100], C[3]) and np.array_equal(C[129], C[7])
    d = ref.sqdist(X, C)
    lab = d.argmin(1)
    assert (lab[rows["on5"]] == 5).all() and (lab[rows["on3"]] == 3).all() and (lab[rows["on7"]] == 7).all() and (lab[rows["mid"]] == 40).all()
    assert (d[rows["on5"], 17] == d[rows["on5"], 5]).all() and (d[rows["on3"], 100] == d[rows["on3"], 3]).all()
    assert (d[rows["on7"], 129] == d[rows["on7"], 7]).all() and (d[rows["mid"], 41] == d[rows["mid"], 40]).all()
    assert not np.isin(lab, [17, 100, 129]).any()
    # float64 holds these integers exactly; so does f32: the largest partial sum is 36 * 64 < 2^24
    assert 36 * 64 < 2 ** 24
