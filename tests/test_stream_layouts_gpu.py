"""The solver's launches under forced gather-ordered and split layouts.

Which arrays and which kernel mode serve a plan is decided per caller
(stream_layout, csrc/aijhip_kernels.hip): MatMult / MatMultAdd, the CG's
SpMV with the fused dot, and the fused V-cycle / set-up ops each take the
packed, 32-bit sorted or coded arrays under conditions of their own and the
original aj / aa otherwise. Every choice computes the same products and sums
them in the same order, so CG + Jacobi (the fused dot) and CG + GAMG (the
fused smoothers on the fine level) must give the plain layout's iteration
count, residual history and solution BIT FOR BIT. Unsplit column codes are
covered by test_column_codes_gpu.py::test_cg_and_gamg_with_codes_bitwise."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PLAIN = dict(gather_sort=0, column_codes=0, row_patterns=0, value_codes=0)
FAR = 1 << 20  # columns this far apart do not fit the packed form's 20 bits


@pytest.fixture(scope="module")
def dev(pkg):
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def assert_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape
    bad = np.nonzero(a.view(np.uint64) != b.view(np.uint64))[0]
    assert bad.size == 0, f"{bad.size}/{a.size} entries differ bitwise; first {bad[:4]}: {a[bad[:4]]} vs {b[bad[:4]]}"


def spd_csr(m, r, c, v):
    """CSR of B + B^T + D for the off-diagonal entries B = (r, c, v) (r != c;
    duplicates summed), D = 1 + the row sums of |B + B^T|: symmetric and
    strictly diagonally dominant."""
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    assert np.all(r != c)
    key = np.concatenate([r * m + c, c * m + r])
    v = np.concatenate([v, v])
    o = np.argsort(key, kind="stable")
    key, v = key[o], v[o]
    first = np.nonzero(np.concatenate([[True], key[1:] != key[:-1]]))[0]
    key, v = key[first], np.add.reduceat(v, first)
    diag = 1.0 + np.bincount(key // m, weights=np.abs(v), minlength=m)
    key = np.concatenate([key, np.arange(m, dtype=np.int64) * (m + 1)])
    v = np.concatenate([v, diag])
    o = np.argsort(key, kind="stable")
    key, v = key[o], v[o]
    ai = np.concatenate([[0], np.cumsum(np.bincount(key // m, minlength=m))]).astype(np.int32)
    return ai, (key % m).astype(np.int32), v


def far_pairs_csr():
    """n = 2^21 rows: the diagonal (4) and -1 at column (i +- 2^20) mod n (one
    column: the two coincide), so every row block spans >= 2^20 columns and
    none takes the packed form. Symmetric, diagonally dominant."""
    n = 2 * FAR
    i = np.arange(n, dtype=np.int64)
    lo = i < FAR
    aj = np.empty(2 * n, np.int32)
    aa = np.empty(2 * n)
    aj[0::2] = np.where(lo, i, i - FAR)
    aj[1::2] = np.where(lo, i + FAR, i)
    aa[0::2] = np.where(lo, 4.0, -1.0)
    aa[1::2] = np.where(lo, -1.0, 4.0)
    return (2 * np.arange(n + 1)).astype(np.int32), aj, aa


def banded_far_csr():
    """A tridiagonal band of 2^20 + 4096 rows and one coupling 2^20 + 100
    columns from the diagonal: the two row blocks that hold it (of ~2000) are
    too wide for the packed form, the others take it."""
    m = FAR + 4096
    i = np.arange(m - 1, dtype=np.int64)
    r = np.concatenate([i, [100]])
    c = np.concatenate([i + 1, [FAR + 200]])
    return spd_csr(m, r, c, np.concatenate([np.full(m - 1, -1.0), [-0.25]]))


def poisson_hub_rows_csr(pkg):
    """test_column_codes_gpu.py::test_split_coded_and_uncoded_blocks' operand
    (50^3 Poisson, a row of 300 scattered extra columns every 25,000 rows: its
    blocks exceed their code dictionaries), plus its transpose and a dominant
    diagonal."""
    ai, aj, aa = pkg.poisson_csr(50)
    m = len(ai) - 1
    rng = np.random.default_rng(3)
    r, c, v = [np.repeat(np.arange(m), np.diff(ai))], [aj.astype(np.int64)], [aa]
    for i in range(17, m, 25000):
        extra = np.setdiff1d(rng.choice(m, 300, replace=False), aj[ai[i]:ai[i + 1]])
        r.append(np.full(len(extra), i))
        c.append(extra)
        v.append(rng.uniform(-1, 1, len(extra)))
    r, c, v = np.concatenate(r), np.concatenate(c), np.concatenate(v)
    off = r != c
    return spd_csr(m, r[off], c[off], v[off])


def has_wide_blocks(A):
    """A plan makes its side stream (long_overlap = 1) only for wide blocks or
    long rows."""
    A.set_option("long_overlap", 1)
    inf = A.info()
    A.set_option("long_overlap", 0)
    return inf["n_long_rows"] == 0 and inf["long_overlap"] == 1


def layout_bytes_over_csr(A):
    inf = A.info()
    return inf["mult_layout_bytes"] - inf["mult_bytes"]


def check_packed(A):  # unsplit: a base column per block beside the 12 B per entry
    assert A.info()["gather_sorted"] == 2 and not has_wide_blocks(A)
    assert layout_bytes_over_csr(A) == 4 * A.info()["n_blocks"]


def check_sorted32(A):  # 14 B per entry
    assert A.info()["gather_sorted"] == 1
    assert layout_bytes_over_csr(A) == 2 * A.info()["nz"]


def check_packed_split(A):  # a base column per narrow block; under a tenth of the blocks wide
    assert A.info()["gather_sorted"] == 2 and has_wide_blocks(A)
    n_wide = A.info()["n_blocks"] - layout_bytes_over_csr(A) // 4
    assert 0 < 10 * n_wide < A.info()["n_blocks"]


def check_codes_split(A):
    assert A.info()["column_codes"] == 1 and has_wide_blocks(A)


# name: (operand, options of both runs, the forced layout's options, its check, MatMult against the oracle)
CASES = {
    "packed": (lambda pkg: pkg.poisson_csr(16), dict(geometry=6), dict(gather_sort=1), check_packed, False),
    "sorted32": (lambda pkg: far_pairs_csr(), dict(geometry=6), dict(gather_sort=1), check_sorted32, False),
    # the fused ops fall back to aj / aa, MatMult keeps the packed copy
    "packed_geometry1": (lambda pkg: pkg.poisson_csr(16), dict(geometry=1), dict(gather_sort=1), check_packed, False),
    # the dot and the fused ops take aj / aa, MatMult the split launch
    "packed_split": (lambda pkg: banded_far_csr(), dict(geometry=6), dict(gather_sort=1), check_packed_split, True),
    "codes_split": (poisson_hub_rows_csr, dict(geometry=6, exact=1), dict(column_codes=1), check_codes_split, True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_solver_on_forced_layout_bitwise(pkg, dev, coracle, name):
    K = importlib.import_module("petsc-openacc_amd.ksp")
    operand, common, forced, check, oracle = CASES[name]
    ai, aj, aa = operand(pkg)
    m = len(ai) - 1
    x = pkg.splitmix_uniform(m, 42)
    b = torch.from_numpy(pkg.splitmix_uniform(m, 7)).to(dev)
    out = {}
    common = {**PLAIN, "long_overlap": 0, **common}  # (no side stream: has_wide_blocks leaves it off too)
    for layout, opts in (("plain", common), ("forced", {**common, **forced})):
        with pkg.SeqAIJHIP(ai, aj, aa, **opts) as A:
            info = A.info()
            assert info["stream_geometry"] == common["geometry"] and info["row_patterns"] == 0
            assert info["value_codes"] == 0 and info["n_long_rows"] == 0
            if layout == "forced":
                check(A)
            else:
                assert (info["gather_sorted"], info["column_codes"]) == (0, 0) and layout_bytes_over_csr(A) == 0
            y = torch.full((m,), np.nan, dtype=torch.float64, device=dev)
            A.mult(torch.from_numpy(x).to(dev), y)
            torch.cuda.synchronize()
            res = [y.cpu().numpy()]
            for pc, kw in (("jacobi", dict(rtol=1e-10)), ("gamg", dict(rtol=1e-14, atol=1e-12))):
                xs = torch.zeros_like(b)
                with K.KSPCG(A, pc=pc, max_it=20, **kw) as ksp:
                    ksp.set_up()
                    ksp.solve(b, xs)
                    torch.cuda.synchronize()
                    assert ksp.fused
                    res += [np.array([ksp.its], dtype=np.float64), ksp.history(), xs.cpu().numpy()]
            out[layout] = res
    assert len(out["plain"]) == len(out["forced"])
    for p, f in zip(out["plain"], out["forced"]):
        assert_bits(p, f)
    if oracle:
        assert_bits(out["forced"][0], coracle.matmult(ai, aj, aa, x, omp=True))
