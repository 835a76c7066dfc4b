"""tests/quality_ref.py (the numpy reference of the sample-quality numbers) against cases worked out by hand."""
import math

import numpy as np

import quality_ref as Q


def test_three_points_on_a_line():
    """x = (0, 1, 3) on a line against itself (self excluded) and against y = (1, 5), sigma^2 = 1/2 and 2:
    exp(-d2 / (2 sigma^2)) = exp(-d2) and exp(-d2 / 4)."""
    x = np.array([[0.0], [1.0], [3.0]])
    y = np.array([[1.0], [5.0]])
    ksum, nn_d2, nn_idx, d2s = Q.pairwise_stats(x, [x, y], [0.5, 2.0], self_group=0)
    assert np.array_equal(d2s[0], [[0, 1, 9], [1, 0, 4], [9, 4, 0]])
    assert np.array_equal(d2s[1], [[1, 25], [0, 16], [4, 4]])
    e = math.exp
    want = [[[e(-1) + e(-9), e(-0.25) + e(-2.25)], [e(-1) + e(-25), e(-0.25) + e(-6.25)]],
            [[e(-1) + e(-4), e(-0.25) + e(-1.0)], [1 + e(-16), 1 + e(-4.0)]],
            [[e(-9) + e(-4), e(-2.25) + e(-1.0)], [2 * e(-4), 2 * e(-1.0)]]]
    np.testing.assert_allclose(ksum, want, rtol=1e-15)
    assert np.array_equal(nn_d2, [[1, 1], [1, 0], [4, 4]])
    assert np.array_equal(nn_idx, [[1, 0], [0, 0], [1, 0]])  # row 2 against y: a tie, the smaller column
    # without the exclusion the diagonal enters: k = 1 more, nearest = itself
    k2, d2, i2, _ = Q.pairwise_stats(x, [x], [0.5])
    np.testing.assert_allclose(k2[:, 0, 0], ksum[:, 0, 0] + 1.0, rtol=1e-15)
    assert np.array_equal(d2[:, 0], [0, 0, 0]) and np.array_equal(i2[:, 0], [0, 1, 2])


def test_one_point_against_itself_has_no_neighbour():
    x = np.array([[2.0, -1.0]])
    ksum, nn_d2, nn_idx, _ = Q.pairwise_stats(x, [x], [1.0, 3.0], self_group=0)
    assert np.array_equal(ksum, np.zeros((1, 1, 2)))
    assert nn_d2[0, 0] == np.inf and nn_idx[0, 0] == -1


def test_sigma0_is_the_mean_over_distinct_pairs():
    rng = np.random.default_rng(3)
    r = rng.normal(1.5, 2.0, (23, 7))
    d2 = Q.sqdist(r, r)
    brute = d2.sum() / (23 * 22)  # the diagonal is zero
    assert abs(Q.sigma0_sq(r) - brute) <= 1e-12 * brute
    bw = Q.bandwidths(r)
    assert len(bw) == 5 and bw[2] == Q.sigma0_sq(r) and bw[0] == bw[2] / 4 and bw[4] == bw[2] * 4


def test_a_set_against_itself():
    """x = y: the nearest point of the other set is the point itself at d2 = 0, so no own neighbour is strictly
    closer (accuracy 0, ties count as wrong), and with S = sum_{i != j} k_ij the estimate is
    2 S / (n (n - 1)) - 2 (S + n) / n^2."""
    rng = np.random.default_rng(5)
    x = rng.normal(0, 1, (9, 4))
    rep = Q.two_sample(x, x.copy())
    assert rep["nn_accuracy"] == {"x": 0.0, "y": 0.0, "all": 0.0}
    assert rep["nn_other"] == {"mean": 0.0, "median": 0.0, "min": 0.0}
    d2 = Q.sqdist(x, x)
    for l, s2 in enumerate(Q.bandwidths(x)):
        k = np.exp(-d2 / (2 * s2))
        S = k.sum() - 9
        want = 2 * S / (9 * 8) - 2 * (S + 9) / 81
        assert abs(rep["mmd2"][l] - want) <= 1e-14
        assert want < 0  # the unbiased form of one sample against itself is below zero
    assert rep["mmd2_at_sigma0"] == rep["mmd2"][2]
    assert abs(rep["sigma0"] ** 2 - Q.sigma0_sq(x)) <= 1e-12 * Q.sigma0_sq(x)


def test_two_far_clusters_are_told_apart():
    rng = np.random.default_rng(7)
    x = rng.normal(0, 1, (12, 5))
    y = rng.normal(0, 1, (10, 5)) + 100.0
    rep = Q.two_sample(x, y)
    assert rep["nn_accuracy"] == {"x": 1.0, "y": 1.0, "all": 1.0}
    # the cross term vanishes: the within-set means remain
    assert rep["mmd2_at_sigma0"] > 0.1
    assert abs(rep["nn_other"]["min"] - math.sqrt(Q.sqdist(x, y).min() / 5)) <= 1e-12
    # one distribution, two samples: near zero against the separated case
    z = rng.normal(0, 1, (10, 5))
    assert abs(Q.two_sample(x, z)["mmd2_at_sigma0"]) < 0.1
