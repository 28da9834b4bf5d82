"""KSPMatSolve (aijhip_ksp_mat_solve): k CG recurrences in lock step on
MatMatMult. The specification is the single-vector solver on its unfused path
(p.w from a pass of its own), reached here through a second handle of the same
operator with the SCALAR kernel: column j of a mat_solve must equal that
handle's KSPCG.solve on column j BIT FOR BIT — X, iteration count, reason,
residual norm and the whole residual history. Nothing here is a tolerance.

The cases: columns that stop at different times (the mask, the freeze, the
column that ends at iteration 0), every chunk width and the 8-byte path of an
odd k, both layouts with padding, a solve cut short inside the first poll
batch, a nonzero initial guess, breakdowns and a NaN beside good columns, the
second stride of the capped vector grid, the host form, the getters, the work
vectors' regrowth, and the other two MatMatMult paths."""
import importlib
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = Path(__file__).resolve().parent.parent
SENTINEL = -7.25
NORMS = ("preconditioned", "unpreconditioned", "natural")
NO_TEMPLATES = dict(row_templates=0, row_patterns=0, column_codes=0)
SIX = ("rhs", "splitmix", "zeros", "spike", "a_exact", "small_rhs")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).ravel().view(np.uint64)


def assert_bits(a, b, what=""):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape, what
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, f"{what}: {bad.size}/{a.size} entries differ bitwise; first at {bad[:4]}"


class Problem:
    """The N^3 Poisson operand (optionally made indefinite), its named
    right-hand sides, and the oracle: single solves on a SCALAR-kernel handle,
    computed once per (column, settings) and shared."""

    def __init__(self, pkg, dev, N, indefinite=False):
        self.pkg, self.dev, self.N = pkg, dev, N
        self.K = importlib.import_module("petsc-openacc_amd.ksp")
        ai, aj, aa = pkg.poisson_csr(N)
        if indefinite:  # the diagonal negated on even rows
            aa = aa.copy()
            rows = np.repeat(np.arange(len(ai) - 1), np.diff(ai))
            aa[(aj == rows) & (rows % 2 == 0)] *= -1.0
        self.csr = (ai, aj, aa)
        self.m = m = len(ai) - 1
        rhs, exact = pkg.poisson_vectors(N)
        self.A_ref = pkg.SeqAIJHIP(ai, aj, aa, kernel="scalar")
        a_exact = torch.empty(m, dtype=torch.float64, device=dev)
        self.A_ref.mult(torch.from_numpy(exact).to(dev), a_exact)
        spike = np.zeros(m)
        spike[m // 2] = 3.0
        nan_rhs = rhs.copy()
        nan_rhs[m // 3] = np.nan
        self.cols = {"rhs": rhs, "splitmix": pkg.splitmix_uniform(m, 42), "zeros": np.zeros(m), "spike": spike,
                     "a_exact": a_exact.cpu().numpy(), "small_rhs": 1e-3 * rhs, "nan_rhs": nan_rhs}
        for v in self.cols.values():
            v.setflags(write=False)
        self._ref = {}

    def operand(self, **options):
        kernel = options.pop("kernel", "auto")
        return self.pkg.SeqAIJHIP(*self.csr, kernel=kernel, **options)

    def guess(self, j):
        return self.pkg.splitmix_uniform(self.m, 1000 + j)

    def ref(self, name, j, pc, norm, rtol, max_it, guess):
        """(x, its, reason, rnorm, history) of the single solve of column `name`
        (initial guess: column j's, when guess is set)."""
        key = (name, j if guess else -1, pc, norm, rtol, max_it)
        if key not in self._ref:
            b = torch.tensor(self.cols[name]).to(self.dev)
            x = torch.from_numpy(self.guess(j)).to(self.dev) if guess else \
                torch.full((self.m,), SENTINEL, dtype=torch.float64, device=self.dev)
            with self.K.KSPCG(self.A_ref, rtol=rtol, max_it=max_it, pc=pc, norm=norm, guess_nonzero=guess) as ksp:
                ksp.solve(b, x)
                torch.cuda.synchronize()
                assert ksp.fused is False  # the unfused path is the specification
                self._ref[key] = (x.cpu().numpy(), ksp.its, ksp.reason, ksp.rnorm, ksp.history().copy())
        return self._ref[key]


@pytest.fixture(scope="module")
def dev(pkg):
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def problems(pkg, dev):
    cache = {}

    def get(N, indefinite=False):
        if (N, indefinite) not in cache:
            cache[(N, indefinite)] = Problem(pkg, dev, N, indefinite)
        return cache[(N, indefinite)]
    return get


def dense_block(rows, k, layout, pad, dev, fill):
    """(buffer, view, ld, inside): a rows x k block of the layout in a flat
    buffer filled with `fill`, its leading dimension padded (interleaved k + 1,
    columns rows + 3) or tight; inside = the buffer indices of the block."""
    ld = (k + 1 if pad else k) if layout == "interleaved" else (rows + 3 if pad else rows)
    count = rows * ld if layout == "interleaved" else k * ld
    buf = torch.full((count,), fill, dtype=torch.float64, device=dev)
    view = buf.view(rows, ld)[:, :k] if layout == "interleaved" else buf.view(k, ld).t()[:rows, :]
    i, j = np.meshgrid(np.arange(rows), np.arange(k), indexing="ij")
    inside = (i * ld + j if layout == "interleaved" else i + j * ld).ravel()
    return buf, view, ld, inside


def check_solve(prob, ksp, names, pc, norm, rtol, max_it, guess=False, layout="interleaved", pad=False, host=False):
    """One mat_solve of the named columns on `ksp` against the single solves.
    Returns the per-column results."""
    m, k, dev = prob.m, len(names), prob.dev
    Bh = np.stack([prob.cols[n] for n in names], axis=1)
    X0 = np.stack([prob.guess(j) for j in range(k)], axis=1) if guess else None
    if host:
        B = np.array(Bh, order="C" if layout == "interleaved" else "F")
        X = np.array(X0 if guess else np.full((m, k), SENTINEL), order="C" if layout == "interleaved" else "F")
        ksp.mat_solve_host(B, X)
        Xh = X
    else:
        _, B, _, _ = dense_block(m, k, layout, pad, dev, np.nan)  # B's padding is NaN and must not matter
        B.copy_(torch.from_numpy(Bh).to(dev))
        xbuf, X, _, inside = dense_block(m, k, layout, pad, dev, SENTINEL)
        if guess:
            X.copy_(torch.from_numpy(X0).to(dev))
        ksp.mat_solve(B, X)
        torch.cuda.synchronize()
        xh = xbuf.cpu().numpy()
        outside = np.ones(xh.size, dtype=bool)
        outside[inside] = False
        assert outside.sum() == xh.size - m * k
        assert np.all(xh[outside] == SENTINEL), "mat_solve wrote outside the m x k block of X"
        Xh = xh[inside].reshape(m, k)
        assert_bits(B.cpu().numpy(), Bh, "B was modified")
    res = ksp.mat_results()
    assert len(res) == k
    for j, name in enumerate(names):
        x, its, reason, rnorm, hist = prob.ref(name, j, pc, norm, rtol, max_it, guess)
        what = f"column {j} ({name}), pc {pc}, norm {norm}"
        print(what, "its", res[j][0], "/", its, "reason", res[j][1], "/", reason)
        assert res[j][0] == its and res[j][1] == reason, (what, res[j], its, reason)
        assert_bits([res[j][2]], [rnorm], what + " rnorm")
        mine = ksp.mat_history(j)
        assert len(mine) == len(hist) == its + 1
        # DIVERGED_INDEFINITE_MAT stops inside iteration `its` and
        # DIVERGED_INDEFINITE_PC at its top, before its norm is logged: the
        # single solver's entry `its` is whatever its history buffer held (it is
        # never written); the logged norms are compared
        logged = its if reason in (-8, -10) else its + 1
        assert_bits(mine[:logged], hist[:logged], what + " history")
        if reason in (-8, -10):
            assert mine[its] == 0.0
        assert_bits(Xh[:, j], x, what + " X")
    # the single-vector getters report the last column
    assert (ksp.its, ksp.reason) == res[-1][:2]
    assert_bits([ksp.rnorm], [res[-1][2]])
    assert_bits(ksp.history(), ksp.mat_history(k - 1))
    return res


def make_ksp(prob, A, pc, norm, rtol, max_it, guess=False):
    return prob.K.KSPCG(A, rtol=rtol, max_it=max_it, pc=pc, norm=norm, guess_nonzero=guess)


# 1 ---- columns that stop at different times
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("pc", ["none", "jacobi"])
@pytest.mark.parametrize("N", [6, 12])
def test_columns_stop_at_different_times(pkg, dev, problems, N, pc, norm):
    """N = 6: one partial block; N = 12: 7 blocks, the last partial. The zero
    column ends at iteration 0, the others at two or three different counts."""
    prob = problems(N)
    with prob.operand() as A, make_ksp(prob, A, pc, norm, 1e-10, 10000) as ksp:
        res = check_solve(prob, ksp, SIX, pc, norm, 1e-10, 10000)
        assert ksp.host_syncs >= 2
    its = [r[0] for r in res]
    assert len(set(its)) > 1, its  # otherwise nothing is masked
    assert res[2][:2] == (0, 3) and res[2][2] == 0.0  # zeros: CONVERGED_ATOL at once
    assert all(r[1] in (2, 3) for r in res), res
    assert max(its) > 8  # more than one poll batch


# 2 ---- widths and chunking
@pytest.mark.parametrize("k", [1, 2, 3, 5, 8, 11])
def test_widths_and_chunks(pkg, dev, problems, k):
    """11 cuts into 8, 2, 1; 3 and 5 have an odd leading dimension: 8-byte accesses."""
    prob = problems(12)
    names = [SIX[j % len(SIX)] for j in range(k)]
    assert pkg.chunk_widths(11) == [8, 2, 1]
    with prob.operand() as A, make_ksp(prob, A, "jacobi", "preconditioned", 1e-10, 10000) as ksp:
        check_solve(prob, ksp, names, "jacobi", "preconditioned", 1e-10, 10000)


# 3 ---- layouts and padding
@pytest.mark.parametrize("layout,pad", [("interleaved", False), ("interleaved", True), ("columns", False),
                                        ("columns", True)])
def test_layouts_and_padding(pkg, dev, problems, layout, pad):
    prob = problems(6)
    names = SIX[:4]
    with prob.operand() as A, make_ksp(prob, A, "jacobi", "preconditioned", 1e-10, 10000) as ksp:
        check_solve(prob, ksp, names, "jacobi", "preconditioned", 1e-10, 10000, layout=layout, pad=pad)
    with prob.operand() as A, make_ksp(prob, A, "none", "natural", 1e-10, 10000, guess=True) as ksp:
        check_solve(prob, ksp, names, "none", "natural", 1e-10, 10000, guess=True, layout=layout, pad=pad)


# 4 ---- cut short inside the first poll batch
def cut_short(pkg, dev, prob):
    """max_it = 3: every nonzero column ends with DIVERGED_ITS at its = 3 and
    has its deferred X += a P applied. Returns the host syncs of the solve."""
    with prob.operand() as A, make_ksp(prob, A, "jacobi", "preconditioned", 1e-10, 3) as ksp:
        res = check_solve(prob, ksp, SIX, "jacobi", "preconditioned", 1e-10, 3)
        for j, name in enumerate(SIX):
            assert res[j][:2] == ((0, 3) if name == "zeros" else (3, -3)), (name, res[j])
        return ksp.host_syncs


def test_cut_short(pkg, dev, problems):
    syncs = cut_short(pkg, dev, problems(6))
    if "AIJHIP_KSP_POLL" not in os.environ:
        assert syncs == 3  # the first poll, the poll after the batch of 3, the final read


CHILD = r"""
import importlib, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import torch
import test_ksp_matsolve_gpu as T
pkg = importlib.import_module("petsc-openacc_amd")
dev = torch.device("cuda:0")
print("syncs", T.cut_short(pkg, dev, T.Problem(pkg, dev, 6)))
"""


def test_cut_short_polling_every_iteration(pkg, dev):
    """The same with AIJHIP_KSP_POLL=1, in a child process of its own."""
    env = dict(os.environ, AIJHIP_KSP_POLL="1")
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=str(ROOT), tests=str(ROOT / "tests"))],
                       capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "syncs 5" in r.stdout, r.stdout  # four polls (one per iteration and the last) and the final read


# 5 ---- nonzero initial guess
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("pc", ["none", "jacobi"])
def test_nonzero_initial_guess(pkg, dev, problems, pc, norm):
    prob = problems(6)
    names = ("rhs", "zeros", "spike")
    with prob.operand() as A, make_ksp(prob, A, pc, norm, 1e-10, 10000, guess=True) as ksp:
        check_solve(prob, ksp, names, pc, norm, 1e-10, 10000, guess=True)


# 6 ---- bad columns beside good ones
@pytest.mark.parametrize("pc", ["none", "jacobi"])
def test_indefinite_operator(pkg, dev, problems, pc):
    """Every column carries its single solve's breakdown reason and bits; an
    INDEFINITE_MAT column does not receive that iteration's X update."""
    prob = problems(6, indefinite=True)
    names = ("rhs", "splitmix", "spike", "zeros")
    with prob.operand() as A, make_ksp(prob, A, pc, "preconditioned", 1e-10, 10000) as ksp:
        res = check_solve(prob, ksp, names, pc, "preconditioned", 1e-10, 10000)
    reasons = [r[1] for r in res]
    assert -10 in reasons and reasons[3] == 3, reasons
    assert all(r in (-8, -10, 3) for r in reasons), reasons


def test_nan_column_beside_good_ones(pkg, dev, problems):
    prob = problems(6)
    names = ("rhs", "nan_rhs", "splitmix", "spike")
    with prob.operand() as A, make_ksp(prob, A, "jacobi", "preconditioned", 1e-10, 10000) as ksp:
        res = check_solve(prob, ksp, names, "jacobi", "preconditioned", 1e-10, 10000)
    assert res[1][:2] == (0, -9) and np.isnan(res[1][2])
    assert all(r[1] == 2 and r[0] > 8 for j, r in enumerate(res) if j != 1), res


# 7 ---- the second stride of the capped vector grid
def test_grid_stride_wrap(pkg, dev, problems):
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    one_stride = 8 * n_cu * 256
    N = 1
    while N ** 3 <= one_stride:
        N += 1
    N += 1  # 256 CUs: 82, 551,368 rows against 524,288
    prob = problems(N)
    assert prob.m > one_stride
    with prob.operand() as A, make_ksp(prob, A, "jacobi", "preconditioned", 1e-10, 20) as ksp:
        res = check_solve(prob, ksp, ("rhs", "splitmix", "a_exact"), "jacobi", "preconditioned", 1e-10, 20)
    assert all(r[:2] == (20, -3) for r in res), res


# 8 ---- host form, getters, regrowth, refusals
@pytest.mark.parametrize("layout", ["interleaved", "columns"])
def test_host_form(pkg, dev, problems, layout):
    prob = problems(6)
    with prob.operand() as A, make_ksp(prob, A, "jacobi", "preconditioned", 1e-10, 10000) as ksp:
        check_solve(prob, ksp, SIX[:5], "jacobi", "preconditioned", 1e-10, 10000, layout=layout, host=True)
    with prob.operand() as A, make_ksp(prob, A, "jacobi", "preconditioned", 1e-10, 10000, guess=True) as ksp:
        check_solve(prob, ksp, SIX[:3], "jacobi", "preconditioned", 1e-10, 10000, guess=True, layout=layout, host=True)


def test_solve_after_mat_solve_and_regrowth(pkg, dev, problems):
    """A following solve equals a fresh handle's; a narrower and then a wider
    mat_solve on the same handle (work vectors reused, then regrown) give the
    single solves' bits as a fresh handle does."""
    prob = problems(12)
    args = ("jacobi", "preconditioned", 1e-10, 10000)
    b = torch.tensor(prob.cols["splitmix"]).to(dev)
    with prob.operand() as A, make_ksp(prob, A, *args) as ksp:
        check_solve(prob, ksp, SIX[:4], *args)
        x = torch.empty_like(b)
        ksp.solve(b, x)
        torch.cuda.synchronize()
        after = (x.cpu().numpy(), ksp.its, ksp.reason, ksp.rnorm, ksp.history().copy())
        check_solve(prob, ksp, SIX[:2], *args)
        check_solve(prob, ksp, [SIX[j % 6] for j in range(9)], *args)
        ksp.set_tolerances(1e-10, 1e-50, 1e5, 20000)  # a longer history
        check_solve(prob, ksp, SIX[:3], "jacobi", "preconditioned", 1e-10, 20000)
    with prob.operand() as A, make_ksp(prob, A, *args) as fresh:
        x = torch.empty_like(b)
        fresh.solve(b, x)
        torch.cuda.synchronize()
        assert (fresh.its, fresh.reason) == after[1:3]
        assert_bits(x.cpu().numpy(), after[0], "solve after mat_solve")
        assert_bits([fresh.rnorm], [after[3]])
        assert_bits(fresh.history(), after[4])


def test_refusals_on_a_live_handle(pkg, dev, problems):
    prob = problems(6)
    m = prob.m
    L = prob.K._lib()
    B = torch.ones(m, 4, dtype=torch.float64, device=dev)
    X = torch.full((m, 4), SENTINEL, dtype=torch.float64, device=dev)
    with prob.operand() as A:
        with prob.K.KSPCG(A, pc="gamg") as ksp:
            with pytest.raises(pkg.AIJHIPError) as e:
                ksp.mat_solve(B, X)
            assert e.value.code == pkg.AIJHIP_ERR_STATE and "V-cycle" in str(e.value)
        with prob.K.KSPCG(A, pc="jacobi") as ksp:
            ksp.mat_solve(B[:, :0], X[:, :0])  # k = 0: nothing happens
            torch.cuda.synchronize()
            assert torch.all(X == SENTINEL)
            bp, xp = B.data_ptr(), X.data_ptr()
            bad = (
                lambda: L.aijhip_ksp_mat_solve(ksp._h, -1, 1, bp, 4, xp, 4, None),
                lambda: L.aijhip_ksp_mat_solve(ksp._h, 65, 1, bp, 65, xp, 65, None),
                lambda: L.aijhip_ksp_mat_solve(ksp._h, 4, 7, bp, 4, xp, 4, None),
                lambda: L.aijhip_ksp_mat_solve(ksp._h, 4, 1, bp, 3, xp, 4, None),
                lambda: L.aijhip_ksp_mat_solve(ksp._h, 4, 0, bp, m, xp, m - 1, None),
                lambda: L.aijhip_ksp_mat_solve(ksp._h, 4, 1, None, 4, xp, 4, None),
                lambda: L.aijhip_ksp_mat_solve(ksp._h, 4, 1, bp, 4, None, 4, None),
                lambda: L.aijhip_ksp_mat_solve(ksp._h, 4, 1, bp, 4, bp, 4, None),
                lambda: L.aijhip_ksp_mat_solve(ksp._h, 2, 1, bp, 4, bp + 8, 4, None),  # columns 0-1 and 1-2
                lambda: L.aijhip_ksp_mat_solve(ksp._h, 2, 0, bp, m, bp + 8 * m, m + 1, None),
                lambda: L.aijhip_ksp_mat_solve_host(ksp._h, 4, 1, None, 4, None, 4),
            )
            for call in bad:
                assert call() == pkg.AIJHIP_ERR_ARG
                assert pkg.lib().aijhip_last_error()
            torch.cuda.synchronize()
            assert torch.all(X == SENTINEL)
            # two column ranges of one interleaved array are distinct blocks
            W = torch.full((m, 4), SENTINEL, dtype=torch.float64, device=dev)
            W[:, :2] = torch.from_numpy(np.stack([prob.cols["rhs"], prob.cols["spike"]], axis=1)).to(dev)
            ksp.mat_solve(W[:, :2], W[:, 2:])
            torch.cuda.synchronize()
            res = ksp.mat_results()
            assert [r[1] for r in res] == [2, 2]


# 9 ---- the other MatMatMult paths
@pytest.mark.parametrize("plan", ["csr", "generic"])
def test_other_plans(pkg, dev, problems, plan):
    prob = problems(12)
    options = NO_TEMPLATES if plan == "csr" else dict(kernel="scalar")
    with prob.operand() as A0:
        assert A0.mat_mult_plan(6)["path"] == 2  # what every other case here runs on
    with prob.operand(**options) as A, make_ksp(prob, A, "jacobi", "preconditioned", 1e-10, 10000) as ksp:
        assert A.mat_mult_plan(6)["path"] == (1 if plan == "csr" else 0)
        res = check_solve(prob, ksp, SIX, "jacobi", "preconditioned", 1e-10, 10000)
    assert len({r[0] for r in res}) > 1


# 10 ---- the bytes of an iteration
@pytest.mark.parametrize("plan", ["templates", "csr", "generic"])
@pytest.mark.parametrize("pc", ["none", "jacobi"])
def test_bytes(pkg, dev, problems, plan, pc):
    """bytes = MatMatMult's plan bytes at k interleaved columns + 88 m k, and
    for Jacobi 8 m per chunk (include/aijhip_ksp.h); at k = 1 no less than the
    single solver's iteration less the 16 m its fused dot saves."""
    prob = problems(12)
    m = prob.m
    options = {"templates": {}, "csr": NO_TEMPLATES, "generic": dict(kernel="scalar")}[plan]
    with prob.operand(**options) as A, make_ksp(prob, A, pc, "preconditioned", 1e-10, 100) as ksp:
        with pytest.raises(pkg.AIJHIPError) as e:
            ksp.mat_solve_bytes(4)
        assert e.value.code == pkg.AIJHIP_ERR_STATE  # not set up yet
        ksp.set_up()
        assert A.info()["m"] == m
        for k in (0, 1, 2, 7, 8, 11, 64):
            sp = A.mat_mult_plan(k, "interleaved")["bytes"]
            chunks = len(pkg.chunk_widths(k))
            total, spmm = ksp.mat_solve_bytes(k)
            assert spmm == sp
            assert total == sp + 88 * m * k + (8 * m * chunks if pc == "jacobi" else 0)
        single = ksp.iteration_bytes()[0]
        assert ksp.mat_solve_bytes(1)[0] >= single - 16 * m
        with pytest.raises(pkg.AIJHIPError):
            ksp.mat_solve_bytes(65)
