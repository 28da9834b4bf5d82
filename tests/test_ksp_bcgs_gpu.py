"""KSPBCGS (AIJHIP_KSP_BCGS) on the GPU against the numpy restatement of the
specified algorithm (tests/bcgs_reference.py) on convection-diffusion operands:
the Poisson operator with its column row - 1 entries times (1 + c) and its
column row + 1 entries times (1 - c); c = 0.3 (stays on row templates), c per
row from default_rng(1).uniform(0, 0.5) (leaves them) and c = 0 (symmetric).

Parity criteria (rtol 1e-10, atol 1e-50): the same reason, iteration counts
within 2, residual-history entries 0..10 within rtol 1e-8 and a true residual
of at most 1e-8 |b| (oracle.seqaij.matmult). Later history entries are not
compared: BiCGStab amplifies another summation order quickly (a CPU run of
the restatement with its dots summed in 256-wide strided blocks: at most 3e-12
over entries 0..10, 4e-7 by entry 30, iteration counts within 1).

Largest deviations measured on an MI355X: test_parity_with_the_restatement's
docstring; with GAMG (N = 16, c = 0 and 0.1) history entries 0..10 within
2.0e-13, equal iteration counts (27 and 19), true residual 3.5e-9 |b|."""
import importlib
import re
import subprocess

import numpy as np
import pytest

import bcgs_reference as ref
from conftest import ROOT
from oracle import seqaij

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = -7.25
TOL = dict(rtol=1e-10, atol=1e-50)
CS = {"c0.3": 0.3, "variable": "variable", "c0": 0.0, "c0.1": 0.1}
_cache = {}
# main_ksp's result block (tests/test_main_ksp.py)
BLOCK = re.compile(r"\[Nx, Ny, Nz\]: \[(\d+), (\d+), (\d+)\]\n"
                   r"Number of iterations: (\d+)\n"
                   r"L2 norm of final residual: (\S+)\n"
                   r"Maximum norm of error: (\S+)\n"
                   r"Time \[init, create solver, solve\]: \[(\S*?), (\S*?), (\S*?)\]")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).ravel().view(np.uint64)


@pytest.fixture(scope="module")
def K(pkg):
    return importlib.import_module("petsc-openacc_amd.ksp")


@pytest.fixture(scope="module")
def dev(pkg):
    return torch.device("cuda", 0)


def system(pkg, N, cname):
    """(ai, aj, aa, b) of the N^3 operand, made once."""
    key = ("sys", N, cname)
    if key not in _cache:
        ai, aj, aa = pkg.poisson_csr(N)
        aa = ref.convection_csr(ai, aj, aa, CS[cname])
        b = pkg.poisson_vectors(N)[0].copy()
        for v in (ai, aj, aa, b):
            v.setflags(write=False)
        _cache[key] = (ai, aj, aa, b)
    return _cache[key]


def restatement(pkg, N, cname, pc, x0=None, **kw):
    """The restatement's (x, its, reason, hist) on the host, made once per case."""
    key = ("ref", N, cname, pc, None if x0 is None else x0.tobytes(), tuple(sorted(kw.items())))
    if key not in _cache:
        ai, aj, aa, b = system(pkg, N, cname)
        dinv = ref.jacobi_inverse(ai, aj, aa)
        _cache[key] = ref.bcgs(lambda y: seqaij.matmult(ai, aj, aa, y),
                               (lambda y: dinv * y) if pc == "jacobi" else (lambda y: y), b, x0=x0,
                               **{**TOL, **kw})
    return _cache[key]


def device_solve(pkg, K, dev, csr, b, pc, kernel="auto", x0=None, **kw):
    """(x, its, reason, rnorm, hist, host_syncs) of one KSPBCGS solve."""
    ai, aj, aa = csr
    A = pkg.SeqAIJHIP(ai, aj, aa, kernel=kernel)
    bd = torch.tensor(np.asarray(b)).to(dev)
    x = torch.full((len(b),), SENTINEL, dtype=torch.float64, device=dev) if x0 is None else \
        torch.tensor(x0).to(dev)
    with K.KSPBCGS(A, pc=pc, guess_nonzero=x0 is not None, **{**TOL, **kw}) as ksp:
        assert ksp.ksp_type == "bcgs" and not ksp.fused
        ksp.solve(bd, x)
        out = (x.cpu().numpy(), ksp.its, ksp.reason, ksp.rnorm, ksp.history(), ksp.host_syncs)
    A.destroy()
    return out


def assert_parity(got, want, csr, b, what):
    x, its, reason, rnorm, hist, _ = got
    xr, its_r, reason_r, hist_r = want
    n = min(11, len(hist), len(hist_r))
    dev_hist = float(np.max(np.abs(hist[:n] - hist_r[:n]) / np.maximum(np.abs(hist_r[:n]), 1e-300)))
    res = float(np.linalg.norm(b - seqaij.matmult(*csr, x)) / np.linalg.norm(b))
    print(f"{what}: its {its} (restatement {its_r}), reason {reason}, history[0..{n - 1}] deviation {dev_hist:.3e}, "
          f"true residual {res:.3e} |b|")
    assert reason == reason_r, what
    assert abs(its - its_r) <= 2, what
    assert len(hist) == its + 1 and hist[-1] == rnorm
    np.testing.assert_allclose(hist[:n], hist_r[:n], rtol=1e-8, atol=0.0, err_msg=what)
    assert res <= 1e-8, what
    return dev_hist, res


@pytest.mark.parametrize("kernel", ["auto", "scalar"])
@pytest.mark.parametrize("pc", ["none", "jacobi"])
@pytest.mark.parametrize("cname", ["c0.3", "variable", "c0"])
def test_parity_with_the_restatement(pkg, K, dev, cname, pc, kernel):
    """N = 12: 1728 rows, 6.75 blocks of 256. Measured on an MI355X over the
    twelve cases: history entries 0..10 deviate by at most 2.4e-11 (relative;
    variable c, PC none), iteration counts by at most 2 (c = 0, Jacobi: 66
    against 68), the true residual is at most 9.5e-11 |b|. The automatic
    layout and the scalar kernel gave the same figures in every case."""
    N = 12
    ai, aj, aa, b = system(pkg, N, cname)
    want = restatement(pkg, N, cname, pc)
    assert want[2] == ref.CONVERGED_RTOL
    got = device_solve(pkg, K, dev, (ai, aj, aa), b, pc, kernel)
    assert_parity(got, want, (ai, aj, aa), b, f"{cname} {pc} {kernel}")


def test_single_partial_block(pkg, K, dev):
    """N = 5: 125 rows, one block of partials."""
    ai, aj, aa, b = system(pkg, 5, "c0.3")
    for pc in ("none", "jacobi"):
        got = device_solve(pkg, K, dev, (ai, aj, aa), b, pc)
        assert_parity(got, restatement(pkg, 5, "c0.3", pc), (ai, aj, aa), b, f"N=5 {pc}")


def test_one_by_one_takes_the_exact_exit(pkg, K, dev):
    """[2] x = [1] with Jacobi: s = 0 and t = 0, so d2 = 0 and s.s = 0; the exit
    applies x += alpha p."""
    csr = (np.array([0, 1], np.int32), np.array([0], np.int32), np.array([2.0]))
    x, its, reason, rnorm, hist, _ = device_solve(pkg, K, dev, csr, np.array([1.0]), "jacobi")
    assert (its, reason, rnorm) == (1, ref.CONVERGED_RTOL, 0.0)
    assert x[0] == 0.5 and hist.tolist() == [0.5, 0.0]


def test_two_by_two_breakdown(pkg, K, dev):
    """[[0, 1], [-1, 0]], b = (1, 0), PC none: v.rp = 0 in the first iteration."""
    csr = (np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32), np.array([1.0, -1.0]))
    x, its, reason, rnorm, hist, _ = device_solve(pkg, K, dev, csr, np.array([1.0, 0.0]), "none")
    assert (its, reason) == (0, K.DIVERGED_BREAKDOWN)
    assert not x.any() and hist.tolist() == [1.0]


def test_edge_cases(pkg, K, dev):
    ai, aj, aa, b = system(pkg, 12, "c0.3")
    csr = (ai, aj, aa)
    x, its, reason, rnorm, hist, _ = device_solve(pkg, K, dev, csr, np.zeros_like(b), "jacobi")
    assert (its, reason, rnorm) == (0, ref.CONVERGED_ATOL, 0.0) and not x.any()
    x, its, reason, rnorm, hist, _ = device_solve(pkg, K, dev, csr, b, "jacobi", max_it=0)
    assert (its, reason) == (0, ref.DIVERGED_ITS) and not x.any() and len(hist) == 1
    want = restatement(pkg, 12, "c0.3", "jacobi", rtol=0.0, max_it=7)
    x, its, reason, rnorm, hist, _ = device_solve(pkg, K, dev, csr, b, "jacobi", rtol=0.0, max_it=7)
    assert (its, reason) == (7, ref.DIVERGED_ITS) and len(hist) == 8
    assert (want[1], want[2]) == (7, ref.DIVERGED_ITS)
    np.testing.assert_allclose(hist, want[3], rtol=1e-8)
    np.testing.assert_allclose(x, want[0], rtol=1e-8, atol=1e-8 * np.abs(want[0]).max())


def test_nonzero_initial_guess(pkg, K, dev):
    ai, aj, aa, b = system(pkg, 12, "c0.3")
    csr = (ai, aj, aa)
    x0 = np.random.default_rng(7).standard_normal(len(b))
    for pc in ("none", "jacobi"):
        want = restatement(pkg, 12, "c0.3", pc, x0=x0)
        assert want[2] == ref.CONVERGED_RTOL
        got = device_solve(pkg, K, dev, csr, b, pc, x0=x0)
        assert_parity(got, want, csr, b, f"guess {pc}")
        # from the converged x the n = 0 test stops the solve. The residual is
        # formed again from x here, so it equals the recurrence's only to
        # rounding: the restart is tested at rtol 1e-8, which the solve to
        # 1e-10 has reached with two digits to spare.
        again = device_solve(pkg, K, dev, csr, b, pc, x0=got[0], rtol=1e-8)
        assert (again[1], again[2]) == (0, ref.CONVERGED_RTOL)
        assert np.array_equal(bits(again[0]), bits(got[0]))


def test_solves_repeat_bit_for_bit_and_under_poll_1(pkg, K, dev, monkeypatch):
    ai, aj, aa, b = system(pkg, 12, "variable")
    csr = (ai, aj, aa)
    monkeypatch.delenv("AIJHIP_KSP_POLL", raising=False)
    first = device_solve(pkg, K, dev, csr, b, "jacobi")
    second = device_solve(pkg, K, dev, csr, b, "jacobi")
    monkeypatch.setenv("AIJHIP_KSP_POLL", "1")
    polled = device_solve(pkg, K, dev, csr, b, "jacobi")
    for other in (second, polled):
        assert np.array_equal(bits(other[0]), bits(first[0]))
        assert np.array_equal(bits(other[4]), bits(first[4]))
        assert other[1:3] == first[1:3]
    its = first[1]
    assert first[5] == 1 + -(-its // 8) + 1  # the first poll, one per batch of 8, the final read
    assert polled[5] == its + 2


def gamg_case(pkg, K, dev, cname):
    """BiCGStab + GAMG at N = 16 against the restatement whose PC is the same
    handle's pc_apply, and the Jacobi solve of the same operand."""
    N = 16
    ai, aj, aa, b = system(pkg, N, cname)
    A = pkg.SeqAIJHIP(ai, aj, aa)
    bd = torch.tensor(b).to(dev)
    x = torch.full((len(b),), SENTINEL, dtype=torch.float64, device=dev)
    with K.KSPBCGS(A, pc="gamg", **TOL) as ksp:
        def pc(y):
            r = torch.tensor(np.ascontiguousarray(y)).to(dev)
            z = torch.empty_like(r)
            ksp.pc_apply(r, z)
            return z.cpu().numpy()
        want = ref.bcgs(lambda y: seqaij.matmult(ai, aj, aa, y), pc, b, **TOL)
        ksp.solve(bd, x)
        got = (x.cpu().numpy(), ksp.its, ksp.reason, ksp.rnorm, ksp.history(), ksp.host_syncs)
        assert ksp.setup_counts()[:2] == (1, 0) and len(ksp.pc_levels()[0]) > 1
    A.destroy()
    assert want[2] == ref.CONVERGED_RTOL
    assert_parity(got, want, (ai, aj, aa), b, f"gamg {cname}")
    jac = device_solve(pkg, K, dev, (ai, aj, aa), b, "jacobi")
    assert jac[2] == ref.CONVERGED_RTOL and got[1] < jac[1], (got[1], jac[1])


def test_gamg_symmetric(pkg, K, dev):
    gamg_case(pkg, K, dev, "c0")


def test_gamg_convection(pkg, K, dev):
    gamg_case(pkg, K, dev, "c0.1")


def test_type_changes_keep_the_pc(pkg, K, dev):
    ai, aj, aa, b = system(pkg, 16, "c0")
    A = pkg.SeqAIJHIP(ai, aj, aa)
    bd = torch.tensor(b).to(dev)

    def solve(ksp):
        x = torch.full((len(b),), SENTINEL, dtype=torch.float64, device=dev)
        ksp.solve(bd, x)
        return x.cpu().numpy(), ksp.its, ksp.reason, ksp.history()

    with K.KSPCG(A, pc="gamg", **TOL) as ksp:
        assert ksp.ksp_type == "cg"
        cg1 = solve(ksp)
        assert ksp.setup_counts()[:2] == (1, 0)
        ksp.set_type("bcgs")
        assert ksp.ksp_type == "bcgs" and ksp.setup_counts()[:2] == (1, 0)
        bc = solve(ksp)
        assert bc[2] == ref.CONVERGED_RTOL and ksp.setup_counts()[:2] == (1, 0)
        assert np.linalg.norm(b - seqaij.matmult(ai, aj, aa, bc[0])) <= 1e-8 * np.linalg.norm(b)
        ksp.set_type("cg")
        cg2 = solve(ksp)
        assert ksp.ksp_type == "cg" and ksp.setup_counts()[:2] == (1, 0)
    A.destroy()
    assert cg1[2] > 0 and cg1[1:3] == cg2[1:3]
    assert np.array_equal(bits(cg1[0]), bits(cg2[0])) and np.array_equal(bits(cg1[3]), bits(cg2[3]))


def test_refusals(pkg, K, dev):
    ai, aj, aa, b = system(pkg, 5, "c0.3")
    A = pkg.SeqAIJHIP(ai, aj, aa)
    bd = torch.tensor(b).to(dev)
    x = torch.zeros_like(bd)
    with K.KSPBCGS(A) as ksp:
        B, X = bd.reshape(-1, 1).clone(), torch.zeros(len(b), 1, dtype=torch.float64, device=dev)
        with pytest.raises(pkg.AIJHIPError) as e:
            ksp.mat_solve(B, X)
        assert e.value.code == pkg.AIJHIP_ERR_STATE and "CG" in str(e.value)
        with pytest.raises(pkg.AIJHIPError) as e:
            ksp.mat_solve_host(np.ones((len(b), 1)), np.zeros((len(b), 1)))
        assert e.value.code == pkg.AIJHIP_ERR_STATE
        with pytest.raises(pkg.AIJHIPError) as e:
            ksp.set_type(7)
        assert e.value.code == pkg.AIJHIP_ERR_ARG and "7" in str(e.value)
        assert ksp.ksp_type == "bcgs"
    with K.KSPBCGS(A, norm="unpreconditioned") as ksp:
        with pytest.raises(pkg.AIJHIPError) as e:
            ksp.solve(bd, x)
        assert e.value.code == pkg.AIJHIP_ERR_STATE and "preconditioned norm" in str(e.value)
    A.destroy()


def test_iteration_bytes_is_the_headers_formula(pkg, K, dev):
    ai, aj, aa, b = system(pkg, 12, "c0.3")
    A = pkg.SeqAIJHIP(ai, aj, aa)
    m, a0 = A.m, A.info()["mult_layout_bytes"]
    with K.KSPBCGS(A, pc="jacobi") as ksp:
        ksp.set_up()
        total, spmv, lev0 = ksp.iteration_bytes()
    # two products, and 32 m + 32 m + 24 m + 32 m + 56 m of vector passes
    assert (total, spmv, lev0) == (2 * a0 + 176 * m, 2 * a0, 2 * a0 + 176 * m)
    with K.KSPBCGS(A, pc="none") as ksp:
        ksp.set_up()
        assert ksp.iteration_bytes()[0] == 2 * a0 + 144 * m
    A.destroy()


def test_main_ksp_bcgs(pkg):
    exe = importlib.import_module("petsc-openacc_amd.build").build_main_ksp()
    r = subprocess.run([str(exe), "-ksp_type", "bcgs", "-pc_type", "jacobi", "-da_grid_x", "16", "-da_grid_y", "16",
                        "-da_grid_z", "16"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr  # a diverged reason exits 91
    m = BLOCK.search(r.stdout)
    assert m, r.stdout
    assert [int(m.group(i)) for i in range(1, 4)] == [16, 16, 16] and int(m.group(4)) > 0
    r = subprocess.run([str(exe), "-config", str(ROOT / "configs" / "bcgs_jacobi.info"), "-da_grid_x", "16",
                        "-da_grid_y", "16", "-da_grid_z", "16"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and BLOCK.search(r.stdout), r.stderr
    assert float(BLOCK.search(r.stdout).group(6)) < 0.05  # the discretisation error at h = 1/16
