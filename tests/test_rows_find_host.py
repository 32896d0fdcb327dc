"""mused_amd.rows_find.rows_find, the NumPy statement of the lookup rule that mused_rows_find is pinned to: bit equality of
rows, duplicates handed out in order of position."""
import numpy as np
import pytest

from mused_amd.rows_find import rows_find


def test_duplicates_are_handed_out_in_order():
    a, b = [1.5, -2.0], [0.25, 7.0]
    X = np.array([b, a, b, a, b, a])                       # a held at 1, 3, 5
    assert np.array_equal(rows_find(X, np.array([a, a, a, a])), [1, 3, 5, -1])      # 3 held, 4 asked
    assert np.array_equal(rows_find(X, np.array([a, b, a, [9.0, 9.0], b, b, b])), [1, 0, 3, -1, 2, 4, -1])
    assert np.array_equal(np.sort(rows_find(X, X[::-1])), np.arange(6))             # the rows held: every position once


def test_equality_is_bit_equality():
    X = np.array([[0.0, 1.0], [-0.0, 1.0], [1.0, np.nan], [1.0, 2.0]])
    assert np.array_equal(rows_find(X, np.array([[-0.0, 1.0], [0.0, 1.0], [0.0, -1.0]])), [1, 0, -1])   # signed zeros
    assert np.array_equal(rows_find(X, np.array([[1.0, np.nan]])), [2])             # the same NaN bits
    other_nan = np.array([[1.0, np.nan]])
    other_nan.view(np.int64)[0, 1] ^= 1
    assert np.isnan(other_nan[0, 1]) and np.array_equal(rows_find(X, other_nan), [-1])
    near = np.array([[1.0, np.nextafter(2.0, 3.0)], [np.nextafter(1.0, 0.0), 2.0], [1.0, 2.0]])   # a last-bit difference
    assert np.array_equal(rows_find(X, near), [-1, -1, 3])


def test_empty_sides_and_arguments():
    X = np.arange(6.0).reshape(3, 2)
    out = rows_find(X, np.empty((0, 2)))
    assert out.shape == (0,) and out.dtype == np.int64      # q = 0
    assert np.array_equal(rows_find(np.empty((0, 2)), X), [-1, -1, -1])
    assert np.array_equal(rows_find(X, X.astype(np.float32)), [0, 1, 2])
    with pytest.raises(ValueError):
        rows_find(X, np.zeros((2, 3)))
    with pytest.raises(ValueError):
        rows_find(X, np.zeros(2))
