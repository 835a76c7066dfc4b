"""tests/manifold_ref.py (the numpy float64 reference of svae_op_pairwise_knn and quality.manifold) on cases whose
answers are worked by hand, on its padding and NaN rules, and on the one statistical property the metrics are read
by: density is 1 in expectation for two samples of one distribution."""
import numpy as np
import pytest

import manifold_ref


def test_five_collinear_points_against_three():
    """x = 0, 1, 2, 3, 10 and y = 0, 2, 4 on a line.  k = 1: every r_1(y)^2 = 4, r_1(x)^2 = 1, 1, 1, 1, 49; the
    balls of y hold x with counts 2, 2, 3, 2, 0.  k = 2: r_2(y)^2 = 16, 4, 16, r_2(x)^2 = 4, 1, 1, 4, 64; counts
    3, 3, 3, 3, 0.  Every y sits in a ball of x and holds an x in its own."""
    x = np.array([[0.0], [1.0], [2.0], [3.0], [10.0]])
    y = np.array([[0.0], [2.0], [4.0]])
    np.testing.assert_array_equal(manifold_ref.self_radii(y, [1, 2]), [[4, 16], [4, 4], [4, 16]])
    np.testing.assert_array_equal(manifold_ref.self_radii(x, [1, 2]), [[1, 4], [1, 1], [1, 1], [1, 4], [49, 64]])
    _, inside, bad, _ = manifold_ref.knn_stats(x, [y], 0, radii=[manifold_ref.self_radii(y, [1, 2])])
    np.testing.assert_array_equal(inside[:, 0], [[2, 3], [2, 3], [3, 3], [2, 3], [0, 0]])
    assert not bad.any()
    rep = manifold_ref.manifold(x, y, ks=(1, 2))
    assert rep == {"k": [1, 2], "precision": [0.8, 0.8], "recall": [1.0, 1.0], "density": [9 / 5, 12 / 10],
                   "coverage": [1.0, 1.0], "nonfinite": 0}
    knn, _, _, _ = manifold_ref.knn_stats(x, [y, x], 2, self_group=1)
    np.testing.assert_array_equal(knn[:, 0], [[0, 4], [1, 1], [0, 4], [1, 1], [36, 64]])
    np.testing.assert_array_equal(knn[:, 1], [[1, 4], [1, 1], [1, 1], [1, 4], [49, 64]])


def test_a_permutation_of_the_real_set_scores_one():
    rng = np.random.default_rng(3)
    y = rng.normal(0, 1, (30, 6))
    rep = manifold_ref.manifold(y[rng.permutation(30)], y, ks=(1, 3, 5))
    assert rep["precision"] == [1.0] * 3 and rep["recall"] == [1.0] * 3 and rep["coverage"] == [1.0] * 3
    assert all(d >= 1.0 for d in rep["density"])  # every ball holds its centre and k more points: (k + 1) / k


def test_two_sets_a_hundred_apart_score_zero():
    rng = np.random.default_rng(4)
    x, y = rng.normal(0, 1, (20, 5)), rng.normal(0, 1, (25, 5)) + 100.0
    rep = manifold_ref.manifold(x, y, ks=(1, 5))
    for key in ("precision", "recall", "density", "coverage"):
        assert rep[key] == [0.0, 0.0], key


def test_fewer_than_k_admitted_columns_pad_with_inf():
    x = np.array([[0.0, 0.0], [3.0, 4.0], [6.0, 8.0]])
    knn, inside, bad, _ = manifold_ref.knn_stats(x, [x, x[:1]], 4, radii=[None, np.array([[25.0, np.inf]])],
                                                 self_group=0)
    np.testing.assert_array_equal(knn[:, 0], [[25, 100, np.inf, np.inf], [25, 25, np.inf, np.inf],
                                              [25, 100, np.inf, np.inf]])
    np.testing.assert_array_equal(knn[:, 1], [[0] + [np.inf] * 3, [25] + [np.inf] * 3, [100] + [np.inf] * 3])
    np.testing.assert_array_equal(inside[:, 0], np.zeros((3, 2)))  # a group without radii
    np.testing.assert_array_equal(inside[:, 1], [[1, 1], [1, 1], [0, 1]])  # <= admits the boundary, +inf everything
    assert not bad.any()
    with pytest.raises(ValueError):
        manifold_ref.manifold(x, x, ks=(3,))  # three points have no third other neighbour


def test_a_nan_is_counted_and_enters_nothing_else():
    rng = np.random.default_rng(5)
    x, y = rng.normal(0, 1, (6, 4)), rng.normal(0, 1, (7, 4))
    r = np.full((7, 2), np.inf)
    r[:, 0] = 1.0
    base = manifold_ref.knn_stats(x, [y], 3, radii=[r])
    for badv in (np.nan, np.inf):
        xb = x.copy()
        xb[2, 1] = badv
        knn, inside, bad, _ = manifold_ref.knn_stats(xb, [y], 3, radii=[r])
        assert bad[2, 0] == 7 and np.all(knn[2] == np.inf) and np.all(inside[2] == 0)
        rest = [0, 1, 3, 4, 5]
        assert np.array_equal(knn[rest], base[0][rest]) and np.array_equal(inside[rest], base[1][rest])
        assert not bad[rest].any()
        yb = y.copy()
        yb[4, 0] = badv
        knn, inside, bad, _ = manifold_ref.knn_stats(x, [yb], 3, radii=[r])
        want = manifold_ref.knn_stats(x, [np.delete(y, 4, 0)], 3, radii=[np.delete(r, 4, 0)])
        assert np.all(bad == 1) and np.array_equal(knn, want[0]) and np.array_equal(inside, want[1])
    rn = r.copy()
    rn[3] = np.nan  # a NaN radius admits nothing
    _, inside, _, d2 = manifold_ref.knn_stats(x, [y], 0, radii=[rn])
    np.testing.assert_array_equal(inside[:, 0, 1], np.full(6, 6))
    np.testing.assert_array_equal(inside[:, 0, 0], (np.delete(d2[0], 3, 1) <= 1.0).sum(1))


def test_density_of_two_samples_of_one_gaussian_is_near_one():
    rng = np.random.default_rng(6)
    x, y = rng.normal(0, 1, (400, 8)), rng.normal(0, 1, (400, 8))
    rep = manifold_ref.manifold(x, y, ks=(5,))
    print("density_5 of two N(0, I) samples, n = m = 400, d = 8: %.4f" % rep["density"][0])
    assert abs(rep["density"][0] - 1.0) <= 0.25
    assert rep["precision"][0] > 0.5 and rep["recall"][0] > 0.5 and rep["coverage"][0] > 0.5
