"""The GAMG refresh's numeric-only product (csrc/gamg_device.hip
k_rowprod_numeric) on its own, through aijhip_gamg_diag_rowprod_numeric: C's
pattern comes from the hash product (aijhip_gamg_diag_rowprod) on the operands
of gamg_product_cases.py, the values of A and B are drawn again
(cases.values: +-2^e mantissas, so a changed order or a dropped term changes
bits), and the result is compared bit for bit, columns included, with
oracle/gamg.py::rowprod_ref on the new values."""
import importlib

import numpy as np
import pytest

import gamg_product_cases as cases
from gamg_product_cases import REGIMES, same_bits
from oracle import gamg as ogamg

gpu = pytest.mark.gpu

_ran = {}


def G_():
    return importlib.import_module("petsc-openacc_amd.gamg")


def fresh_values(c, seed):
    """The case's operands with new values on the same structure."""
    rng = np.random.default_rng(seed)
    (ai, aj, aa), (bi, bj, ba) = c["A"], c["B"]
    return (ai, aj, cases.values(rng, len(aa))), (bi, bj, cases.values(rng, len(ba)))


def run_numeric(key, c, seed):
    """((ci, cj, ca), report, A', B') of the numeric product on the pattern the hash product made."""
    if key not in _ran:
        (ci, cj, _), _ = G_().device_rowprod(c["A"], c["B"], c["n"], n_cu=c["n_cu"])
        A2, B2 = fresh_values(c, seed)
        C, report = G_().device_rowprod_numeric(A2, B2, c["n"], ci, cj, n_cu=c["n_cu"])
        _ran[key] = (C, report, A2, B2)
    return _ran[key]


def check_report(report, m):
    """Every launch is an instantiation numeric_classes lists, in write mode,
    its capacity reported as the most columns a row may hold."""
    pairs = set(G_().numeric_classes())
    assert report["passes"]
    for lanes, cap, mode, kmax in report["passes"]:
        assert mode == "write" and kmax == cap and (lanes, cap) in pairs, (lanes, cap, mode, kmax)
    assert len(report["row_table"]) == m


@gpu
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("G", cases.LANES)
def test_numeric_product_family_is_bit_exact(pkg, G, regime):
    """Every hash family: rows of 3 to 1023 distinct columns at every class
    edge of the hash product, A rows of 1, G-1, G, G+1 and 3G+1 entries, empty
    A and B rows, B rows named several times over, all three storage orders."""
    c = cases.hash_family(G, regime)
    C, report, A2, B2 = run_numeric(("family", G, regime), c, 5000 + 10 * G + (regime == "full"))
    assert report["shape"] == (c["m"], c["n"])
    assert same_bits(C, ogamg.rowprod_ref(A2, B2))
    check_report(report, c["m"])


@gpu
@pytest.mark.parametrize("regime", REGIMES)
def test_numeric_product_probing_case(pkg, regime):
    """Columns up to INT32_MAX - 1 (the rank search compares them as signed
    32-bit), rows that fill each class."""
    c = cases.probing_case(regime)
    C, report, A2, B2 = run_numeric(("probing", regime), c, 77 + (regime == "full"))
    assert same_bits(C, ogamg.rowprod_ref(A2, B2))
    assert C[1].max() == 2**31 - 2
    check_report(report, c["m"])


@gpu
def test_every_numeric_instantiation_ran(pkg):
    """Over the families and the probing cases, every (lanes, capacity) pair
    the kernel is instantiated for was launched."""
    ran = set()
    for G in cases.LANES:
        for regime in REGIMES:
            c = cases.hash_family(G, regime)
            ran |= {p[:2] for p in run_numeric(("family", G, regime), c, 5000 + 10 * G + (regime == "full"))[1]["passes"]}
    for regime in REGIMES:
        ran |= {p[:2] for p in run_numeric(("probing", regime), cases.probing_case(regime), 77 + (regime == "full"))[1]["passes"]}
    want = set(G_().numeric_classes())
    assert want and want <= ran, sorted(want - ran)
    # the classes cover every row the hash product covers (up to 1023 columns)
    assert max(cap for _, cap in want) >= 1023
    assert all(64 % lanes == 0 and 1 <= lanes <= 64 for lanes, _ in want)


def _csr(rows, vals):
    ai = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int32)
    aj = np.concatenate([np.asarray(r, np.int64) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int32)
    return ai, aj, np.asarray(vals, np.float64)


@gpu
def test_a_row_names_one_b_row_twice(pkg):
    """The second naming adds to the slots the first one filled, in order."""
    rng = np.random.default_rng(3)
    B = _csr([[5, 1, 9], [2, 5], [0]], cases.values(rng, 6))
    A = _csr([[0, 1, 0], [1, 1, 1, 2], [0]], cases.values(rng, 8))
    ci, cj, ca = want = ogamg.rowprod_ref(A, B)
    C, report = G_().device_rowprod_numeric(A, B, 10, ci, cj)
    assert same_bits(C, want)
    check_report(report, 3)


@gpu
def test_empty_rows_of_a_and_b(pkg):
    """An empty A row (nothing written, nothing read past it) and an empty B
    row named by a non-empty A row (a step without products)."""
    rng = np.random.default_rng(4)
    B = _csr([[3, 0], [], [7, 3, 1]], cases.values(rng, 5))
    A = _csr([[], [1, 0, 1], [1], [2, 1, 0]], cases.values(rng, 7))
    want = ogamg.rowprod_ref(A, B)
    assert np.diff(want[0]).tolist() == [0, 2, 0, 4]
    C, report = G_().device_rowprod_numeric(A, B, 8, want[0], want[1])
    assert same_bits(C, want)


@gpu
def test_product_of_no_rows(pkg):
    B = _csr([[0, 1]], [1.0, 2.0])
    empty = (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    (ci, cj, ca), report = G_().device_rowprod_numeric(empty, B, 2, np.zeros(1, np.int32), np.zeros(0, np.int32))
    assert ci.tolist() == [0] and len(cj) == 0 and len(ca) == 0 and report["shape"] == (0, 2)
    assert report["passes"] == []


@gpu
def test_pattern_column_no_product_reaches_is_plus_zero(pkg):
    """One extra column in the pattern of each row (before, between and after
    the columns reached): +0.0 with the sign bit clear; the others keep their
    bits. The products of row 1 are negative, so a slot that took one would
    show."""
    B = _csr([[2, 6], [4]], [-1.5, -2.5, -3.0])
    A = _csr([[0, 1], [0], [1]], [2.0, 4.0, 1.0, 8.0])
    ci, cj, ca = ogamg.rowprod_ref(A, B)
    assert cj.tolist() == [2, 4, 6, 2, 6, 4]
    pi = np.array([0, 4, 7, 9], np.int32)
    pj = np.array([2, 3, 4, 6, 0, 2, 6, 4, 9], np.int32)  # extras: 3 (between), 0 (before), 9 (after)
    (gi, gj, ga), _ = G_().device_rowprod_numeric(A, B, 10, pi, pj)
    assert np.array_equal(gi, pi) and np.array_equal(gj, pj)
    extra = np.array([1, 4, 8])
    assert np.array_equal(ga[extra].view(np.uint64), np.zeros(3, np.uint64))  # +0.0: all bits clear
    keep = np.setdiff1d(np.arange(9), extra)
    assert np.array_equal(ga[keep].view(np.uint64), ca.view(np.uint64))


@gpu
@pytest.mark.parametrize("width", [1024, 1030])
def test_pattern_row_past_the_largest_class(pkg, width):
    """A row of 1024 or more pattern columns: AIJHIP_ERR_STATE (the refresh
    then takes the level on the host), as the hash product's too-wide row; the
    next product of the process is exact."""
    c = cases.too_wide_case("full")
    ai, aj, aa = c["A"]
    keep = np.ones(len(aj), bool)
    keep[ai[c["row"]]:ai[c["row"] + 1]] = False
    A = (np.concatenate(([0], np.cumsum(np.where(np.arange(c["m"]) == c["row"], 0, np.diff(ai))))).astype(np.int32),
         aj[keep], aa[keep])
    ci, cj, ca = want = ogamg.rowprod_ref(A, c["B"])
    # the emptied row's pattern: `width` columns nothing reaches
    at = ci[c["row"]]
    wide_j = np.concatenate((cj[:at], np.arange(width, dtype=np.int32), cj[at:]))
    wide_i = ci.copy()
    wide_i[c["row"] + 1:] += width
    with pytest.raises(pkg.AIJHIPError) as e:
        G_().device_rowprod_numeric(A, c["B"], c["n"], wide_i, wide_j)
    assert e.value.code == pkg.AIJHIP_ERR_STATE and "largest class" in str(e.value)
    # 1023 columns go through (all +0.0), and the others are exact
    ok_j = np.concatenate((cj[:at], np.arange(1023, dtype=np.int32), cj[at:]))
    ok_i = ci.copy()
    ok_i[c["row"] + 1:] += 1023
    (gi, gj, ga), report = G_().device_rowprod_numeric(A, c["B"], c["n"], ok_i, ok_j)
    assert not ga[at:at + 1023].view(np.uint64).any()
    assert np.array_equal(np.delete(ga, np.arange(at, at + 1023)).view(np.uint64), ca.view(np.uint64))
    assert 1024 in {cap for _, cap, _, _ in report["passes"]}


@gpu
def test_malformed_pattern_is_refused(pkg):
    B = _csr([[0, 1]], [1.0, 2.0])
    A = _csr([[0]], [3.0])
    for ci, cj in (([0, 2], [1, 0]), ([0, 2], [0, 0]), ([0, 1], [2]), ([1, 2], [0])):
        with pytest.raises((pkg.AIJHIPError, ValueError)) as e:
            G_().device_rowprod_numeric(A, B, 2, np.array(ci, np.int32), np.array(cj, np.int32))
        if isinstance(e.value, pkg.AIJHIPError):
            assert e.value.code == pkg.AIJHIP_ERR_ARG
