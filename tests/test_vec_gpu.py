"""include/aijhip_vec.h called directly (through ksp.DeviceVecOps), not only
inside KSPCGMPI solves of a few thousand rows per rank: sizes around the wave
and workgroup widths, at the grid cap (2048 workgroups x 256 lanes = 524 288
entries) and past it (a second trip of the grid-stride loops, partly filled
last workgroups; from 262 145 entries on, more partials than the finishing
kernel's 1024 lanes), and n = 0.

Elementwise results are compared bit for bit with numpy's expressions of the
same two roundings (the library is built with -ffp-contract=off). Reductions
against math.fsum of the products: a term passes through fewer than 64
roundings on its way into the result (its product, the lane's <= 3 serial
adds at these sizes, 6 shuffle steps, 4 wave sums, then the finishing
kernel's <= 2 serial adds, 6 shuffle steps and 16 wave sums), so
|got - exact| <= 64 * 2^-53 * sum |terms| — derived, not measured."""
import importlib
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

gpu = pytest.mark.gpu
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 524288, 524289, 1048577]
BOUND = 64 * 2.0 ** -53


@pytest.fixture(scope="module")
def K(pkg):
    return importlib.import_module("petsc-openacc_amd.ksp")


@pytest.fixture(scope="module")
def ops(pkg, K):
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return K.DeviceVecOps(torch.device("cuda:0"))


def vectors(n, seed, count):
    """Magnitudes in [0.5, 1] with random signs: no entry is small enough to
    be dropped from a sum unnoticed."""
    rng = np.random.default_rng(seed * 1_000_003 + n)
    return [rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n) for _ in range(count)]


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def bits_equal(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    assert bad.size == 0, f"{bad.size}/{got.size} entries differ bitwise; first {bad[:4]}: {got[bad[:4]]} vs {want[bad[:4]]}"


def check_sum(got, terms):
    exact, scale = math.fsum(terms), math.fsum(np.abs(terms))
    assert abs(got - exact) <= BOUND * scale, (got, exact, abs(got - exact), BOUND * scale)
    if len(terms) == 0:
        assert got == 0.0 and not math.isnan(got)


def reduced(ops, call, k):
    """The first k result slots of a reduction; NaN beforehand, so a slot
    the call leaves alone shows."""
    ops.red.fill_(float("nan"))
    call()
    torch.cuda.synchronize()
    return ops.red.cpu().numpy()[:k].copy()


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_aypx(ops, n):
    x, y = vectors(n, 1, 2)
    beta = -0.8125
    yd = to_dev(y)
    ops.aypx(beta, to_dev(x), yd)
    torch.cuda.synchronize()
    bits_equal(yd.cpu().numpy(), x + beta * y)


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_dot(ops, n):
    x, y = vectors(n, 2, 2)
    xd, yd = to_dev(x), to_dev(y)
    first = reduced(ops, lambda: ops.dot(xd, yd), 1)
    check_sum(float(first[0]), x * y)
    bits_equal(reduced(ops, lambda: ops.dot(xd, yd), 1), first)  # summed in a fixed order


@gpu
@pytest.mark.parametrize("form", ["dinv", "no-dinv", "z-aliases-w"])
@pytest.mark.parametrize("n", SIZES)
def test_cg_update(ops, n, form):
    """x = x + a p; r = r + (-a) w; z = dinv r (or r); z.z, z.r, r.r — with
    z in w's storage as KSPCGMPI calls it (w is read before z is written)."""
    x, p, r, w = vectors(n, 3, 4)
    dinv = None if form == "no-dinv" else np.random.default_rng(n).uniform(0.5, 2.0, n)
    a = 0.37109375
    r1 = r + (-a) * w
    z1 = r1 if dinv is None else dinv * r1
    pd, dd = to_dev(p), None if dinv is None else to_dev(dinv)
    results = []
    for _ in range(2):
        xd, rd, wd = to_dev(x), to_dev(r), to_dev(w)
        zd = wd if form == "z-aliases-w" else torch.full_like(wd, float("nan"))
        results.append(reduced(ops, lambda: ops.cg_update(a, xd, pd, rd, wd, zd, dd), 3))
        bits_equal(xd.cpu().numpy(), x + a * p)
        bits_equal(rd.cpu().numpy(), r1)
        bits_equal(zd.cpu().numpy(), z1)
        if form != "z-aliases-w":
            bits_equal(wd.cpu().numpy(), w)
    for got, terms in zip(results[0], (z1 * z1, z1 * r1, r1 * r1)):
        check_sum(float(got), terms)
    bits_equal(results[1], results[0])


@gpu
@pytest.mark.parametrize("with_dinv", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_jacobi(ops, n, with_dinv):
    (r,) = vectors(n, 4, 1)
    dinv = np.random.default_rng(n + 1).uniform(0.5, 2.0, n) if with_dinv else None
    z1 = dinv * r if with_dinv else r
    rd, dd = to_dev(r), to_dev(dinv) if with_dinv else None
    zd = torch.full_like(rd, float("nan"))
    first = reduced(ops, lambda: ops.jacobi(rd, dd, zd), 3)
    bits_equal(zd.cpu().numpy(), z1)
    bits_equal(rd.cpu().numpy(), r)
    for got, terms in zip(first, (z1 * z1, z1 * r, r * r)):
        check_sum(float(got), terms)
    bits_equal(reduced(ops, lambda: ops.jacobi(rd, dd, zd), 3), first)


def test_bad_arguments_are_refused_before_any_launch(pkg, K):
    """A negative n and a NULL result pointer return AIJHIP_ERR_ARG: the
    checks come before the scratch allocation and the launches, so this
    needs no device (tests/test_abi.py's pattern)."""
    L = K._veclib()
    E = pkg.AIJHIP_ERR_ARG
    assert L.aijhip_vec_aypx(-1, 2.0, None, None, None) == E
    assert L.aijhip_vec_dot(-1, None, None, None, None) == E
    assert L.aijhip_vec_cg_update(-1, 1.0, None, None, None, None, None, None, None, None) == E
    assert L.aijhip_vec_jacobi(-1, None, None, None, None, None) == E
    for n in (0, 4):
        assert L.aijhip_vec_dot(n, None, None, None, None) == E
        assert L.aijhip_vec_cg_update(n, 1.0, None, None, None, None, None, None, None, None) == E
        assert L.aijhip_vec_jacobi(n, None, None, None, None, None) == E
    assert b"bad arguments" in pkg.lib().aijhip_last_error()
