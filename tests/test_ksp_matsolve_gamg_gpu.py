"""KSPMatSolve and PCMatApply with GAMG: the multi-column V-cycle on MatMatMult
with its smoothing epilogues, and the GAMG branch of the lock-step CG.

The specification is the single-vector path: a second handle of the same
operator with the SCALAR kernel (ksp.fused is False) and the same gamg= /
smoother=, KSPCG.pc_apply / KSPCG.solve per column. Both handles' hierarchies
are compared bit for bit first (pc_level, pc_levels); a failure there belongs
to the set-up.

Bits or bars: the single-vector launches reorder a row's sum only for rows
longer than a block's lanes keep in order, and launch_spmm never reorders, so
the longest row over every A_l, P_l and P_l^T is computed here from pc_level.
Up to 128 entries everything is compared bit for bit (the Poisson cases at
N = 8 and 12 must be there); beyond it the fused-against-unfused bars of
test_gamg.py::test_gpu_vcycle_fused_smoothers_bitwise apply: equal iteration
counts and reasons, histories to rtol 1e-12 / atol 1e-15 h[0], X (and a
V-cycle's Z) to rtol 1e-10 / atol 1e-12 max|x|."""
import importlib

import numpy as np
import pytest

from test_ksp_matsolve_gpu import SENTINEL, SIX, assert_bits, bits, dense_block

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NORMS = ("preconditioned", "unpreconditioned", "natural")
SMOOTHERS = {"default": None,
             "richardson2-scale0.9": dict(type="richardson", its=2, scale=0.9),
             "richardson3": dict(type="richardson", its=3),
             "chebyshev1": dict(type="chebyshev", its=1),
             "chebyshev2": dict(type="chebyshev", its=2),
             "chebyshev3": dict(type="chebyshev", its=3)}
PLANS = {"templates": ({}, 2), "csr": (dict(row_templates=0, row_patterns=0, column_codes=0), 1),
         "generic": (dict(kernel="scalar"), 0)}
VCYCLE_COLUMNS = ("rhs", "nan_rhs", "splitmix", "zeros", "spike")
LAYOUTS = [("interleaved", False), ("interleaved", True), ("columns", False), ("columns", True)]


def hierarchy(ksp):
    """([rows], [nnz], [(ai, aj, aa, n) of A_l], [the same of P_l])."""
    rows, nnz, _ = ksp.pc_levels()
    nl = len(rows)
    return rows, nnz, [ksp.pc_level(l, "A") for l in range(nl)], [ksp.pc_level(l, "P") for l in range(nl - 1)]


def assert_same_hierarchy(a, b):
    assert a[0] == b[0] and a[1] == b[1], (a[0], b[0], a[1], b[1])
    for la, lb in zip(a[2] + a[3], b[2] + b[3]):
        assert la[3] == lb[3]
        assert np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1])
        assert_bits(la[2], lb[2], "a level's values")


def longest_row(h):
    """Over every A_l, P_l and P_l^T."""
    longest = 0
    for ai, aj, aa, n in h[2] + h[3]:
        longest = max(longest, int(np.diff(ai).max(initial=0)))
    for ai, aj, aa, n in h[3]:
        longest = max(longest, int(np.bincount(aj, minlength=max(n, 1)).max(initial=0)))
    return longest


class Case:
    """One operand, its named columns, and the oracle: a SCALAR-kernel handle
    per (smoother, solver settings), its V-cycles and solves computed once."""

    def __init__(self, pkg, dev, csr, cols, gamg=None):
        self.pkg, self.dev, self.csr, self.gamg = pkg, dev, csr, gamg
        self.K = importlib.import_module("petsc-openacc_amd.ksp")
        self.m = len(csr[0]) - 1
        self.cols = cols
        for v in cols.values():
            v.setflags(write=False)
        self.A_ref = pkg.SeqAIJHIP(*csr, kernel="scalar")
        self._handles, self._vc, self._solves = {}, {}, {}

    def guess(self, j):
        return self.pkg.splitmix_uniform(self.m, 1000 + j)

    def ref_handle(self, smname, **kw):
        key = (smname, tuple(sorted(kw.items())))
        if key not in self._handles:
            ksp = self.K.KSPCG(self.A_ref, pc="gamg", gamg=self.gamg, smoother=SMOOTHERS[smname], **kw)
            ksp.set_up()
            assert ksp.fused is False  # the unfused path is the specification
            self._handles[key] = (ksp, hierarchy(ksp))
        return self._handles[key]

    def ref_vcycle(self, smname, name):
        if (smname, name) not in self._vc:
            ksp, _ = self.ref_handle(smname)
            r = torch.tensor(self.cols[name]).to(self.dev)
            z = torch.full((self.m,), SENTINEL, dtype=torch.float64, device=self.dev)
            ksp.pc_apply(r, z)
            torch.cuda.synchronize()
            assert_bits(r.cpu().numpy(), self.cols[name], "pc_apply modified r")
            self._vc[smname, name] = z.cpu().numpy()
        return self._vc[smname, name]

    def ref_solve(self, smname, name, j, norm, rtol, max_it, guess):
        key = (smname, name, j if guess else -1, norm, rtol, max_it)
        if key not in self._solves:
            ksp, _ = self.ref_handle(smname, rtol=rtol, max_it=max_it, norm=norm, guess_nonzero=guess)
            b = torch.tensor(self.cols[name]).to(self.dev)
            x = torch.from_numpy(self.guess(j)).to(self.dev) if guess else \
                torch.full((self.m,), SENTINEL, dtype=torch.float64, device=self.dev)
            ksp.solve(b, x)
            torch.cuda.synchronize()
            self._solves[key] = (x.cpu().numpy(), ksp.its, ksp.reason, ksp.rnorm, ksp.history().copy())
        return self._solves[key]

    def handle(self, smname, plan, width, **kw):
        """(A, ksp, exact): a set-up handle on `plan` (None: automatic) whose hierarchy equals
        the oracle's; exact: whether bits are owed (longest row <= 128)."""
        options, path = PLANS[plan] if plan else ({}, None)
        options = dict(options)
        A = self.pkg.SeqAIJHIP(*self.csr, kernel=options.pop("kernel", "auto"), **options)
        assert path is None or A.mat_mult_plan(4)["path"] == path, (plan, A.mat_mult_plan(4))
        ksp = self.K.KSPCG(A, pc="gamg", gamg=self.gamg, smoother=SMOOTHERS[smname], mat_vcycle=width, **kw)
        ksp.set_up()
        h = hierarchy(ksp)
        assert_same_hierarchy(h, self.ref_handle(smname, **kw)[1])
        return A, ksp, longest_row(h) <= 128


def named_columns(m, rhs, splitmix):
    spike = np.zeros(m)
    spike[m // 2] = 3.0
    nan_rhs = rhs.copy()
    nan_rhs[m // 3] = np.nan
    return {"rhs": rhs.copy(), "splitmix": splitmix, "zeros": np.zeros(m), "spike": spike, "nan_rhs": nan_rhs,
            "small_rhs": 1e-3 * rhs}


@pytest.fixture(scope="module")
def dev(pkg):
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cases(pkg, dev):
    cache = {}

    def get(key):
        if key not in cache:
            if isinstance(key, int):
                csr = pkg.poisson_csr(key)
                m = len(csr[0]) - 1
                rhs, exact = pkg.poisson_vectors(key)
                cols = named_columns(m, rhs, pkg.splitmix_uniform(m, 42))
                c = Case(pkg, dev, csr, cols)
                a_exact = torch.empty(m, dtype=torch.float64, device=dev)
                c.A_ref.mult(torch.from_numpy(exact).to(dev), a_exact)
                c.cols["a_exact"] = a_exact.cpu().numpy()
            else:
                from test_templates_solver_gpu import OPERANDS
                import scipy.sparse as sp
                ai, aj, aa = OPERANDS[key][0]()
                m = len(ai) - 1
                rhs = sp.csr_matrix((aa, aj, ai), shape=(m, m)) @ np.random.default_rng(7).standard_normal(m)
                c = Case(pkg, dev, (ai, aj, aa), named_columns(m, rhs, pkg.splitmix_uniform(m, 42)),
                         gamg=dict(coarse_eq_limit=50))
            cache[key] = c
        return cache[key]
    yield get
    for c in cache.values():
        for ksp, _ in c._handles.values():
            ksp.destroy()


def assert_column(got, ref, exact, what):
    """Bits (NaNs where the reference has NaNs), or the bars beyond 128-entry rows."""
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), what + ": NaN entries differ"
    if exact:
        assert_bits(got[~nan], ref[~nan], what)
    else:
        scale = np.abs(ref[~nan]).max(initial=0.0)
        np.testing.assert_allclose(got[~nan], ref[~nan], rtol=1e-10, atol=1e-12 * scale, err_msg=what)


def check_vcycle(case, ksp, smname, names, exact, layout="interleaved", pad=False):
    """pc_mat_apply on the named columns against pc_apply per column."""
    m, k, dev = case.m, len(names), case.dev
    Rh = np.stack([case.cols[n] for n in names], axis=1)
    _, R, _, _ = dense_block(m, k, layout, pad, dev, np.nan)  # R's padding is NaN and must not matter
    R.copy_(torch.from_numpy(Rh).to(dev))
    zbuf, Z, _, inside = dense_block(m, k, layout, pad, dev, SENTINEL)
    ksp.pc_mat_apply(R, Z)
    torch.cuda.synchronize()
    zh = zbuf.cpu().numpy()
    outside = np.ones(zh.size, dtype=bool)
    outside[inside] = False
    assert np.all(zh[outside] == SENTINEL), "pc_mat_apply wrote outside the m x k block of Z"
    got = R.cpu().numpy()
    assert np.array_equal(bits(got), bits(Rh)), "R was modified"
    Zh = zh[inside].reshape(m, k)
    for j, name in enumerate(names):
        assert_column(Zh[:, j], case.ref_vcycle(smname, name), exact,
                      f"column {j} ({name}) of {k}, {smname}, {layout}{' padded' if pad else ''}")


# 1 ---- the V-cycle alone
@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("smname", list(SMOOTHERS))
@pytest.mark.parametrize("N", [8, 12])
def test_vcycle_columns_equal_single_vcycles(pkg, dev, cases, N, smname, plan):
    """Three levels; k = 11 cuts into 8, 2, 1, and 3 and 5 take the 8-byte
    forms; a NaN column beside good ones from k = 2 on; both layouts, tight and
    padded; the six smoothers cover both parities of each rotation and the
    Chebyshev step without p_km1."""
    case = cases(N)
    A, ksp, exact = case.handle(smname, plan, 11)
    with A, ksp:
        assert len(ksp.pc_levels()[0]) == 3
        assert exact, "the Poisson hierarchies at N = 8 and 12 have no row above 128 entries"
        assert pkg.chunk_widths(11) == [8, 2, 1]
        for k in (1, 2, 3, 5, 8, 11):
            names = [VCYCLE_COLUMNS[j % len(VCYCLE_COLUMNS)] for j in range(k)]
            for layout, pad in (LAYOUTS if k in (3, 8) else LAYOUTS[:1]):
                check_vcycle(case, ksp, smname, names, exact, layout, pad)
        # the single V-cycle of this handle (fused launches on its finest plan) too
        r = torch.tensor(case.cols["rhs"]).to(dev)
        z = torch.empty_like(r)
        ksp.pc_apply(r, z)
        torch.cuda.synchronize()
        assert_column(z.cpu().numpy(), case.ref_vcycle(smname, "rhs"), exact, "pc_apply on the test handle")


@pytest.mark.parametrize("pc", ["jacobi", "none"])
def test_pc_apply_jacobi_and_none(pkg, dev, cases, pc):
    case = cases(8)
    ai, aj, aa = case.csr
    rowsof = np.repeat(np.arange(case.m), np.diff(ai))
    diag = np.zeros(case.m)
    diag[rowsof[aj == rowsof]] = aa[aj == rowsof]
    names = ("rhs", "splitmix", "spike")
    Rh = np.stack([case.cols[n] for n in names], axis=1)
    want = (1.0 / diag)[:, None] * Rh if pc == "jacobi" else Rh
    with pkg.SeqAIJHIP(*case.csr) as A, case.K.KSPCG(A, pc=pc) as ksp:
        r = torch.tensor(case.cols["rhs"]).to(dev)
        z = torch.full_like(r, SENTINEL)
        ksp.pc_apply(r, z)
        torch.cuda.synchronize()
        assert_bits(z.cpu().numpy(), want[:, 0], f"pc_apply, {pc}")
        for layout, pad in LAYOUTS:
            _, R, _, _ = dense_block(case.m, 3, layout, pad, dev, np.nan)
            R.copy_(torch.from_numpy(Rh).to(dev))
            zbuf, Z, _, inside = dense_block(case.m, 3, layout, pad, dev, SENTINEL)
            ksp.pc_mat_apply(R, Z)
            torch.cuda.synchronize()
            zh = zbuf.cpu().numpy()
            outside = np.ones(zh.size, dtype=bool)
            outside[inside] = False
            assert np.all(zh[outside] == SENTINEL)
            assert_bits(zh[inside].reshape(case.m, 3), want, f"pc_mat_apply, {pc}, {layout}")


# 2 ---- four levels and non-Poisson rows
@pytest.mark.parametrize("smname", ["default", "chebyshev2"])
@pytest.mark.parametrize("operand", [24, "paired7-empty-rows", "box9-40x37"])
def test_vcycle_four_levels_and_other_rows(pkg, dev, cases, operand, smname):
    case = cases(operand)
    # Poisson on row templates; the stand-ins on their automatic plan, whatever path it takes
    A, ksp, exact = case.handle(smname, "templates" if operand == 24 else None, 4)
    with A, ksp:
        rows = ksp.pc_levels()[0]
        print(f"{operand}: levels {rows}, path {A.mat_mult_plan(4)['path']}, "
              f"{'bitwise' if exact else 'bars (a row above 128 entries)'}")
        if operand == 24:
            assert len(rows) == 4
        check_vcycle(case, ksp, smname, ("rhs", "splitmix", "zeros", "spike"), exact)
        check_vcycle(case, ksp, smname, ("spike", "rhs", "splitmix"), exact, "columns", True)


def check_solve(case, ksp, smname, names, exact, norm, rtol, max_it, guess=False, layout="interleaved", pad=False,
                host=False):
    """One GAMG mat_solve of the named columns against the oracle's single solves."""
    m, k, dev = case.m, len(names), case.dev
    Bh = np.stack([case.cols[n] for n in names], axis=1)
    X0 = np.stack([case.guess(j) for j in range(k)], axis=1) if guess else None
    if host:
        B = np.array(Bh, order="C" if layout == "interleaved" else "F")
        X = np.array(X0 if guess else np.full((m, k), SENTINEL), order="C" if layout == "interleaved" else "F")
        ksp.mat_solve_host(B, X)
        Xh = X
    else:
        _, B, _, _ = dense_block(m, k, layout, pad, dev, np.nan)
        B.copy_(torch.from_numpy(Bh).to(dev))
        xbuf, X, _, inside = dense_block(m, k, layout, pad, dev, SENTINEL)
        if guess:
            X.copy_(torch.from_numpy(X0).to(dev))
        ksp.mat_solve(B, X)
        torch.cuda.synchronize()
        xh = xbuf.cpu().numpy()
        outside = np.ones(xh.size, dtype=bool)
        outside[inside] = False
        assert np.all(xh[outside] == SENTINEL), "mat_solve wrote outside the m x k block of X"
        Xh = xh[inside].reshape(m, k)
        assert np.array_equal(bits(B.cpu().numpy()), bits(Bh)), "B was modified"
    res = ksp.mat_results()
    assert len(res) == k
    for j, name in enumerate(names):
        x, its, reason, rnorm, hist = case.ref_solve(smname, name, j, norm, rtol, max_it, guess)
        what = f"column {j} ({name}), {smname}, norm {norm}"
        print(what, "its", res[j][0], "/", its, "reason", res[j][1], "/", reason)
        assert res[j][0] == its and res[j][1] == reason, (what, res[j], its, reason)
        mine = ksp.mat_history(j)
        assert len(mine) == len(hist) == its + 1
        # reasons -8 / -10 stop before iteration `its` logs its norm (the
        # documented exception of test_ksp_matsolve_gpu.check_solve)
        logged = its if reason in (-8, -10) else its + 1
        if exact:
            assert_column(np.array([res[j][2]]), np.array([rnorm]), True, what + " rnorm")
            assert_column(mine[:logged], hist[:logged], True, what + " history")
        else:
            h0 = abs(hist[0]) if logged and np.isfinite(hist[0]) else 0.0
            np.testing.assert_allclose(mine[:logged], hist[:logged], rtol=1e-12, atol=1e-15 * h0, err_msg=what)
        if reason in (-8, -10):
            assert mine[its] == 0.0
        assert_column(Xh[:, j], x, exact, what + " X")
    assert (ksp.its, ksp.reason) == res[-1][:2]
    return res


# 3 ---- lock-step solves
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("smname", ["default", "chebyshev2"])
@pytest.mark.parametrize("N", [8, 12])
def test_solves_stop_at_different_times(pkg, dev, cases, N, smname, norm):
    case = cases(N)
    kw = dict(rtol=1e-10, max_it=10000, norm=norm)
    A, ksp, exact = case.handle(smname, "templates", 6, **kw)
    with A, ksp:
        assert exact
        res = check_solve(case, ksp, smname, SIX, exact, norm, 1e-10, 10000)
    its = [r[0] for r in res]
    assert len(set(its)) > 1, its  # otherwise nothing is masked
    assert res[2][:2] == (0, 3) and res[2][2] == 0.0  # zeros: CONVERGED_ATOL at once
    assert all(r[1] in (2, 3) for r in res), res


@pytest.mark.parametrize("norm", NORMS)
def test_solves_from_a_nonzero_guess(pkg, dev, cases, norm):
    """The preconditioned and natural norms take the extra V-cycle on B (from
    padded column blocks through the staging block as well)."""
    case = cases(8)
    kw = dict(rtol=1e-10, max_it=10000, norm=norm, guess_nonzero=True)
    A, ksp, exact = case.handle("default", "templates", 3, **kw)
    with A, ksp:
        check_solve(case, ksp, "default", ("rhs", "zeros", "spike"), exact, norm, 1e-10, 10000, guess=True)
        check_solve(case, ksp, "default", ("rhs", "zeros", "spike"), exact, norm, 1e-10, 10000, guess=True,
                    layout="columns", pad=True)


def test_solve_cut_short_inside_the_first_batch(pkg, dev, cases):
    case = cases(8)
    kw = dict(rtol=1e-10, max_it=3, norm="preconditioned")
    A, ksp, exact = case.handle("default", "templates", 6, **kw)
    with A, ksp:
        res = check_solve(case, ksp, "default", SIX, exact, "preconditioned", 1e-10, 3)
    for j, name in enumerate(SIX):
        assert res[j][:2] == ((0, 3) if name == "zeros" else (3, -3)), (name, res[j])


@pytest.mark.parametrize("k", [1, 3, 8, 11])
def test_solve_widths(pkg, dev, cases, k):
    case = cases(12)
    kw = dict(rtol=1e-10, max_it=10000, norm="preconditioned")
    A, ksp, exact = case.handle("default", "templates", k, **kw)
    with A, ksp:
        check_solve(case, ksp, "default", [SIX[j % 6] for j in range(k)], exact, "preconditioned", 1e-10, 10000)


@pytest.mark.parametrize("plan", list(PLANS))
def test_solve_on_the_three_finest_plans(pkg, dev, cases, plan):
    case = cases(12)
    kw = dict(rtol=1e-10, max_it=10000, norm="preconditioned")
    A, ksp, exact = case.handle("chebyshev2", plan, 4, **kw)
    with A, ksp:
        check_solve(case, ksp, "chebyshev2", SIX[:4], exact, "preconditioned", 1e-10, 10000)


def test_solve_host_form_and_layouts(pkg, dev, cases):
    case = cases(8)
    kw = dict(rtol=1e-10, max_it=10000, norm="preconditioned")
    A, ksp, exact = case.handle("default", "templates", 5, **kw)
    with A, ksp:
        check_solve(case, ksp, "default", SIX[:5], exact, "preconditioned", 1e-10, 10000, host=True)
        for layout, pad in LAYOUTS[1:]:
            check_solve(case, ksp, "default", SIX[:4], exact, "preconditioned", 1e-10, 10000, layout=layout, pad=pad)


def test_solve_nan_column_beside_good_ones(pkg, dev, cases):
    case = cases(8)
    kw = dict(rtol=1e-10, max_it=10000, norm="preconditioned")
    A, ksp, exact = case.handle("default", "templates", 4, **kw)
    with A, ksp:
        res = check_solve(case, ksp, "default", ("rhs", "nan_rhs", "splitmix", "spike"), exact, "preconditioned",
                          1e-10, 10000)
    assert res[1][1] == -9 and np.isnan(res[1][2])
    assert all(r[1] == 2 for j, r in enumerate(res) if j != 1), res


# 4 ---- the second stride of the capped vector grid
def test_grid_stride_wrap(pkg, dev, cases):
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    one_stride = 8 * n_cu * 256
    N = 1
    while N ** 3 <= one_stride:
        N += 1
    N += 1  # 256 CUs: 82
    case = cases(N)
    assert case.m > one_stride
    kw = dict(rtol=1e-10, max_it=3, norm="preconditioned")
    A, ksp, exact = case.handle("default", "templates", 3, **kw)
    with A, ksp:
        print(f"N = {N}: levels {ksp.pc_levels()[0]}, {'bitwise' if exact else 'bars'}")
        res = check_solve(case, ksp, "default", ("rhs", "splitmix", "a_exact"), exact, "preconditioned", 1e-10, 3)
    assert all(r[:2] == (3, -3) for r in res), res


# 5 ---- state
def test_default_handle_refuses_and_width_is_checked(pkg, dev, cases):
    case = cases(8)
    m = case.m
    B = torch.ones(m, 4, dtype=torch.float64, device=dev)
    X = torch.full((m, 4), SENTINEL, dtype=torch.float64, device=dev)
    with pkg.SeqAIJHIP(*case.csr) as A:
        with case.K.KSPCG(A, pc="gamg") as ksp:
            assert ksp.mat_vcycle_width == 0
            for call in (ksp.mat_solve, ksp.pc_mat_apply):
                with pytest.raises(pkg.AIJHIPError) as e:
                    call(B, X)
                assert e.value.code == pkg.AIJHIP_ERR_STATE and "V-cycle has no multi-column form" in str(e.value)
            ksp.set_up()
            with pytest.raises(pkg.AIJHIPError) as e:
                ksp.mat_solve_bytes(2)
            assert e.value.code == pkg.AIJHIP_ERR_STATE and "V-cycle" in str(e.value)
        with case.K.KSPCG(A, pc="gamg", mat_vcycle=3) as ksp:
            assert ksp.mat_vcycle_width == 3
            for call in (ksp.mat_solve, ksp.pc_mat_apply):
                with pytest.raises(pkg.AIJHIPError) as e:
                    call(B, X)
                assert e.value.code == pkg.AIJHIP_ERR_STATE
                assert "4" in str(e.value) and "3" in str(e.value), str(e.value)
            with pytest.raises(pkg.AIJHIPError):
                ksp.set_mat_vcycle_width(65)
            torch.cuda.synchronize()
            assert torch.all(X == SENTINEL)


def test_raising_the_width_keeps_the_hierarchy(pkg, dev, cases):
    case = cases(12)
    kw = dict(rtol=1e-10, max_it=10000, norm="preconditioned")
    A, ksp, exact = case.handle("default", "templates", 2, **kw)
    with A, ksp:
        path, seconds = ksp.setup_path(), ksp.pc_levels()[2]
        check_solve(case, ksp, "default", SIX[:2], exact, "preconditioned", 1e-10, 10000)
        ksp.set_mat_vcycle_width(6)
        check_solve(case, ksp, "default", SIX, exact, "preconditioned", 1e-10, 10000)
        check_solve(case, ksp, "default", SIX[:2], exact, "preconditioned", 1e-10, 10000)
        assert ksp.setup_path() == path and ksp.pc_levels()[2] == seconds  # not set up again


def test_single_solve_after_a_gamg_mat_solve(pkg, dev, cases):
    case = cases(12)
    kw = dict(rtol=1e-10, max_it=10000, norm="preconditioned")
    b = torch.tensor(case.cols["splitmix"]).to(dev)
    A, ksp, exact = case.handle("default", "templates", 4, **kw)
    with A, ksp:
        check_solve(case, ksp, "default", SIX[:4], exact, "preconditioned", 1e-10, 10000)
        x = torch.empty_like(b)
        ksp.solve(b, x)
        torch.cuda.synchronize()
        after = (x.cpu().numpy(), ksp.its, ksp.reason, ksp.rnorm, ksp.history().copy())
    with pkg.SeqAIJHIP(*case.csr) as A2, case.K.KSPCG(A2, pc="gamg", **kw) as fresh:
        x = torch.empty_like(b)
        fresh.solve(b, x)
        torch.cuda.synchronize()
        assert (fresh.its, fresh.reason) == after[1:3]
        assert_bits(x.cpu().numpy(), after[0], "solve after a GAMG mat_solve")
        assert_bits([fresh.rnorm], [after[3]])
        assert_bits(fresh.history(), after[4])


def test_bytes_of_a_gamg_iteration(pkg, dev, cases):
    case = cases(12)
    A, ksp, _ = case.handle("default", "csr", 8)
    with A, ksp:
        for k in (1, 2, 8):
            total, product = ksp.mat_solve_bytes(k)
            assert 0 < product < total, (k, total, product)
            assert product > A.mat_mult_plan(k)["bytes"]  # the V-cycle's products beside CG's
        assert ksp.mat_solve_bytes(8)[0] < 8 * ksp.mat_solve_bytes(1)[0]  # the matrices count once per chunk
