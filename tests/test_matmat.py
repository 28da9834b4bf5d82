"""MatMatMult (aijhip_mat_mat_mult, Y = A X for k dense columns): the parts
that need no device — how k columns are cut into launches, the argument
checks that come before any device work, and dense_layout, which reads a
block's layout and leading dimension off its strides."""
import ctypes

import numpy as np
import pytest


def widths_of(pkg, k, cap=None):
    L = pkg.lib()
    cap = k // 8 + 3 if cap is None else cap
    w = (ctypes.c_int32 * max(cap, 1))()
    n = ctypes.c_int32(-1)
    rc = L.aijhip_mat_mat_mult_chunk_widths(k, w, cap, ctypes.byref(n))
    return rc, list(w[:max(n.value, 0)][:cap]), n.value


@pytest.mark.parametrize("k", [0, 1, 7, 8, 9, 19, 64])
def test_chunk_widths(pkg, k):
    """Greedy, largest first, from {8, 4, 2, 1}: the widths sum to k and do not increase."""
    rc, w, n = widths_of(pkg, k)
    assert rc == pkg.AIJHIP_OK and n == len(w)
    assert sum(w) == k
    assert set(w) <= {8, 4, 2, 1}
    assert all(a >= b for a, b in zip(w, w[1:]))
    assert w == [8] * (k // 8) + [b for b in (4, 2, 1) if k & b]
    assert pkg.chunk_widths(k) == w


def test_chunk_widths_examples_and_small_cap(pkg):
    assert pkg.chunk_widths(7) == [4, 2, 1]
    assert pkg.chunk_widths(19) == [8, 8, 2, 1]
    rc, _, n = widths_of(pkg, 19, cap=3)
    assert rc == pkg.AIJHIP_ERR_ARG and n == 4  # the count needed is still reported
    assert b"needed" in pkg.lib().aijhip_last_error()
    rc, _, _ = widths_of(pkg, 7, cap=0)
    assert rc == pkg.AIJHIP_ERR_ARG
    assert pkg.lib().aijhip_mat_mat_mult_chunk_widths(-1, None, 0, None) == pkg.AIJHIP_ERR_ARG
    assert pkg.lib().aijhip_mat_mat_mult_chunk_widths(0, None, 0, None) == pkg.AIJHIP_OK


def test_null_handle(pkg):
    """The three calls that take a handle refuse NULL before any device work."""
    L = pkg.lib()
    x = np.zeros(4)
    y = np.zeros(4)
    calls = (
        lambda: L.aijhip_mat_mat_mult(None, 1, 0, x.ctypes.data, 4, y.ctypes.data, 4, None),
        lambda: L.aijhip_mat_mat_mult_host(None, 1, 1, x.ctypes.data, 1, y.ctypes.data, 1),
        lambda: L.aijhip_mat_mat_mult_get_plan(None, 1, 0, None, None, None),
    )
    for call in calls:
        L.aijhip_mat_mat_mult_chunk_widths(-1, None, 0, None)  # another message in between
        assert call() == pkg.AIJHIP_ERR_ARG
        assert b"NULL" in L.aijhip_last_error()


def elem_strides(a):
    return tuple(s // a.itemsize for s in a.strides)


def test_dense_layout(pkg):
    n, k = 11, 4
    c = np.zeros((n, k))
    assert pkg.dense_layout(c.shape, elem_strides(c)) == ("interleaved", k)
    f = np.zeros((n, k), order="F")
    assert pkg.dense_layout(f.shape, elem_strides(f)) == ("columns", n)
    pr = np.zeros((n, k + 1))[:, :k]  # padded rows
    assert pkg.dense_layout(pr.shape, elem_strides(pr)) == ("interleaved", k + 1)
    pc = np.zeros((n + 3, k), order="F")[:n, :]  # padded columns
    assert pkg.dense_layout(pc.shape, elem_strides(pc)) == ("columns", n + 3)
    # torch's strides are in elements already
    assert pkg.dense_layout((n, k), (k + 1, 1)) == ("interleaved", k + 1)
    assert pkg.dense_layout((n, k), (1, n + 3)) == ("columns", n + 3)


def test_dense_layout_single_column_matches_either(pkg):
    """k = 1 has no second column: any positive row stride is an interleaved
    block, and with unit row stride it is a SeqDense column as well."""
    n = 11
    for a in (np.zeros((n, 1)), np.zeros((n, 1), order="F")):
        lay, ld = pkg.dense_layout(a.shape, elem_strides(a))
        assert (lay, ld) in (("interleaved", 1), ("columns", n))
    wide = np.zeros((n, 5))[:, 2:3]
    assert pkg.dense_layout(wide.shape, elem_strides(wide)) == ("interleaved", 5)
    col = np.zeros((n + 3, 2), order="F")[:n, 1:2]
    # paired with a block of either layout
    for other in (np.zeros((n, 1)), np.zeros((n, 1), order="F"), wide):
        lay, ldx, ldy = pkg._common_dense_layout(col.shape, elem_strides(col), other.shape, elem_strides(other))
        assert lay in (0, 1) and ldx >= 1 and ldy >= 1


def test_dense_layout_rejects_doubly_strided_and_mixed(pkg):
    n, k = 11, 4
    v = np.zeros((2 * n, 2 * k))[::2, ::2]
    with pytest.raises(TypeError):
        pkg.dense_layout(v.shape, elem_strides(v))
    with pytest.raises(TypeError):
        pkg.dense_layout((n, k), (2, 2 * n))
    with pytest.raises(TypeError):
        pkg.dense_layout((n, k), (k - 1, 1))  # rows that overlap
    with pytest.raises(TypeError):
        pkg.dense_layout((n,), (1,))
    c, f = np.zeros((n, k)), np.zeros((n, k), order="F")
    with pytest.raises(TypeError):  # one layout for both
        pkg._common_dense_layout(c.shape, elem_strides(c), f.shape, elem_strides(f))
