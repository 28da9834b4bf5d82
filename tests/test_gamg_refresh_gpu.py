"""GAMG reuse-interpolation (aijhip_ksp_set_gamg_reuse_interpolation): new
values on the structure a GAMG handle was set up on refresh its hierarchy.

What a refresh owes, and what is checked here:
  - setup_counts: one full set-up, then one refresh;
  - every P_l is the first set-up's bit for bit, every A_l pattern unchanged;
  - every A_l, l >= 1, has the bits of the oracle's chain P_l^T (A_l' P_l) on
    the new A_0' and the KEPT P_l: oracle/gamg.py::rowprod_ref at 8^3 and 12^3,
    scipy's products exactly as oracle/gamg.py::build forms them elsewhere
    (equal patterns asserted first);
  - Chebyshev: each level's bounds come from ogamg.estimate_emax_cg on the
    refreshed A_l, bit for bit (the bar tests/test_gamg.py holds the set-up's
    hierarchy, and so its estimate, to);
  - the same values again leave every bit of the hierarchy, the V-cycle and a
    solve as they were; values x 4 scale them by exact powers of two;
  - the V-cycle after a refresh, and mat_solve's columns, equal a SCALAR-kernel
    handle's taken through the same sequence (bits up to 128-entry rows, else
    the bars of test_ksp_matsolve_gamg_gpu.py); the V-cycle also matches
    ogamg.vcycle on the oracle levels.

The new values are A' = S A S, S = diag(u), u uniform in [0.5, 2]: SPD with A,
the same pattern, coefficients no longer constant (row templates fall to row
patterns)."""
import importlib

import numpy as np
import pytest
import scipy.sparse as sp

from gamg_product_cases import same_bits
from oracle import gamg as ogamg
from test_ksp_matsolve_gamg_gpu import (PLANS, SMOOTHERS, VCYCLE_COLUMNS, assert_column, assert_same_hierarchy,
                                        hierarchy, longest_row, named_columns)
from test_ksp_matsolve_gpu import SENTINEL, assert_bits

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

INT32_MAX = 2**31 - 1
DMR = {"device": 0, "host": INT32_MAX}


def K_():
    return importlib.import_module("petsc-openacc_amd.ksp")


def rows_of(ai):
    return np.repeat(np.arange(len(ai) - 1), np.diff(ai))


def sas(csr, seed=11):
    """A' = S A S, S = diag(u), u uniform in [0.5, 2] (seeded)."""
    ai, aj, aa = csr
    u = np.random.default_rng(seed).uniform(0.5, 2.0, len(ai) - 1)
    return (u[rows_of(ai)] * aa) * u[aj]


_operands = {}


def operand(pkg, key):
    """(csr, gamg parameters) of Poisson N^3 with the reference point, or a
    small stand-in from the harness builders."""
    if key not in _operands:
        if isinstance(key, int):
            _operands[key] = (pkg.poisson_csr(key), {})
        elif key == "fem_hex":
            _operands[key] = (pkg.fem_hex_csr(7, 6, 5, dofs=3, seed=1565), {})
        else:
            _operands[key] = (pkg.skewed_csr(3000, seed=7), {})
        for a in _operands[key][0]:
            a.setflags(write=False)
    return _operands[key]


def make(pkg, csr, plan, **kw):
    options = dict(PLANS[plan][0])
    A = pkg.SeqAIJHIP(*csr, kernel=options.pop("kernel", "auto"), **options)
    return A, K_().KSPCG(A, pc="gamg", **kw)


def transpose_csr(P, n):
    """P^T with every row listing P's rows ascending (the set-up's transpose)."""
    pi, pj, pa = P
    order = np.argsort(pj, kind="stable")
    ti = np.concatenate(([0], np.cumsum(np.bincount(pj, minlength=n)))).astype(np.int32)
    return ti, rows_of(pi)[order].astype(np.int32), pa[order]


def oracle_chain(A0, Ps, exact_ref):
    """[A_0', A_1', ...] as CSR triples: A_(l+1)' = P_l^T (A_l' P_l) with the
    kept P_l = (pi, pj, pa, n). exact_ref: rowprod_ref, else scipy as
    oracle/gamg.py::build forms the products."""
    out = [A0]
    for pi, pj, pa, n in Ps:
        A = out[-1]
        m = len(A[0]) - 1
        if exact_ref:
            AP = ogamg.rowprod_ref(A, (pi, pj, pa))
            out.append(ogamg.rowprod_ref(transpose_csr((pi, pj, pa), n), AP))
        else:
            As = sp.csr_matrix((A[2], A[1], A[0]), shape=(m, m))
            P = sp.csr_matrix((pa, pj, pi), shape=(m, n))
            P.sort_indices()
            PT = sp.csr_matrix(P.T)
            PT.sort_indices()
            AP = sp.csr_matrix(As @ P)
            AP.sort_indices()
            Ac = sp.csr_matrix(PT @ AP)
            Ac.sort_indices()
            out.append((Ac.indptr.astype(np.int32), Ac.indices.astype(np.int32), Ac.data))
    return out


def check_refreshed(h0, h1, aa1, exact_ref):
    """h0 / h1: the hierarchy before and after the refresh to values aa1."""
    assert h0[0] == h1[0] and h0[1] == h1[1]
    for p0, p1 in zip(h0[3], h1[3]):  # every P_l kept bit for bit
        assert p0[3] == p1[3] and same_bits(p0[:3], p1[:3])
    for a0, a1 in zip(h0[2], h1[2]):  # every A_l pattern unchanged
        assert np.array_equal(a0[0], a1[0]) and np.array_equal(a0[1], a1[1])
    assert_bits(h1[2][0][2], aa1, "the finest operator's values")
    want = oracle_chain((h1[2][0][0], h1[2][0][1], aa1), h1[3], exact_ref)
    for l in range(1, len(want)):
        got = h1[2][l][:3]
        assert np.array_equal(got[0], want[l][0]) and np.array_equal(got[1], want[l][1]), f"A_{l}: pattern"
        assert_bits(got[2], want[l][2], f"A_{l} after the refresh")


def assert_reserve_kept(ksp, before, what):
    """The multi-column blocks (b, x, r, w per level) and the lock-step work
    vectors (R, Z, P) are the allocations they were: the same device addresses,
    none of them NULL on a handle with a reserved width."""
    now = ksp.mat_vcycle_reserve()
    assert now == before, f"{what}: the multi-column reserve was re-allocated"
    if ksp.mat_vcycle_width > 0:
        assert len(now) == 4 * len(ksp.pc_levels()[0]) + 3 and all(now), now


def refresh_case(pkg, key, where, plan, device_update=False, gamg_extra=None, **kw):
    """Set up with the flag, update to S A S, set up again; returns (A, ksp, h0, h1, aa1)."""
    csr, gamg = operand(pkg, key)
    gamg = dict(gamg, **(gamg_extra or {}))
    if where in DMR:
        gamg["device_min_rows"] = DMR[where]
    A, ksp = make(pkg, csr, plan, gamg=gamg or None, reuse_interpolation=True, **kw)
    assert ksp.reuse_interpolation is True
    ksp.set_up()
    assert ksp.setup_counts()[:2] == (1, 0)
    h0 = hierarchy(ksp)
    reserve = ksp.mat_vcycle_reserve()
    aa1 = sas(csr)
    if device_update:
        A.update_values_device(torch.from_numpy(aa1).cuda())
    else:
        A.update_values(aa1)
    ksp.set_up()
    assert ksp.setup_counts()[:2] == (1, 1), ksp.setup_counts()
    assert_reserve_kept(ksp, reserve, "the refresh")
    ksp.set_up()  # nothing changed since: neither path runs
    assert ksp.setup_counts()[:2] == (1, 1)
    return A, ksp, h0, hierarchy(ksp), aa1


# 1 ---- the hierarchy
@pytest.mark.parametrize("plan", ["templates", "csr", "generic"])
@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("N", [8, 12, 24])
def test_refresh_poisson_hierarchy(pkg, N, where, plan):
    A, ksp, h0, h1, aa1 = refresh_case(pkg, N, where, plan, device_update=(N == 12 and plan == "csr"))
    with A, ksp:
        print(f"{N}^3 {where} {plan}: levels {h1[0]}, path {ksp.setup_path()}")
        assert len(h1[0]) >= 3
        check_refreshed(h0, h1, aa1, exact_ref=N in (8, 12))


@pytest.mark.parametrize("plan", ["templates", "csr", "generic"])
def test_refresh_poisson_12_default_parameters(pkg, plan):
    A, ksp, h0, h1, aa1 = refresh_case(pkg, 12, "default", plan)
    with A, ksp:
        check_refreshed(h0, h1, aa1, exact_ref=True)


@pytest.mark.parametrize("N", [12, 24])
def test_refresh_through_the_host_builder_gives_the_same_bits(pkg, N, monkeypatch):
    """The path a level takes whose rows pass the numeric kernel's classes
    (AIJHIP_GAMG_REFRESH=host sends every level there): the host builder's
    products on operands read back from the level handles."""
    monkeypatch.setenv("AIJHIP_GAMG_REFRESH", "host")
    A, ksp, h0, h1, aa1 = refresh_case(pkg, N, "device", "csr")
    with A, ksp:
        check_refreshed(h0, h1, aa1, exact_ref=N == 12)


@pytest.mark.parametrize("where", ["device", "host"])
def test_two_refreshes_in_a_row(pkg, where):
    """A second update_values + set_up on one handle: the row classes counted by
    the first refresh are reused, and on the host-built hierarchy the numeric
    A P runs on the pattern the first refresh made with the symbolic product
    (kept without values). Both refreshes against the oracle chain; the
    reserve's allocations stay through both."""
    A, ksp, h0, h1, aa1 = refresh_case(pkg, 12, where, "csr", mat_vcycle=3)
    with A, ksp:
        check_refreshed(h0, h1, aa1, exact_ref=True)
        reserve = ksp.mat_vcycle_reserve()
        csr, _ = operand(pkg, 12)
        aa2 = sas(csr, seed=12)
        assert not np.array_equal(aa1, aa2)
        A.update_values(aa2)
        ksp.set_up()
        assert ksp.setup_counts()[:2] == (1, 2)
        check_refreshed(h0, hierarchy(ksp), aa2, exact_ref=True)
        assert_reserve_kept(ksp, reserve, "the second refresh")


@pytest.mark.parametrize("smname,eig_ksp", [("chebyshev1", 1), ("chebyshev2", 1), ("chebyshev1", 0)])
@pytest.mark.parametrize("where", ["device", "host"])
def test_refresh_reestimates_chebyshev_bounds(pkg, where, smname, eig_ksp):
    """mg_smoother(l)'s bounds after the refresh are lo, hi x the set-up's
    estimate on the refreshed A_l and its D^-1 (eig_ksp 1: ogamg.estimate_emax_cg,
    CG's Lanczos; 0: ogamg.estimate_emax, the power iteration); they moved."""
    G = importlib.import_module("petsc-openacc_amd.gamg")
    sm = G.mg_smoother(**SMOOTHERS[smname])
    csr, _ = operand(pkg, 12)
    with pkg.SeqAIJHIP(*csr) as A0, K_().KSPCG(A0, pc="gamg", gamg=dict(device_min_rows=DMR[where], eig_ksp=eig_ksp),
                                                smoother=SMOOTHERS[smname]) as k0:
        k0.set_up()
        before = [k0.mg_smoother(l) for l in range(len(k0.pc_levels()[0]) - 1)]
    A, ksp, h0, h1, aa1 = refresh_case(pkg, 12, where, "templates", gamg_extra=dict(eig_ksp=eig_ksp),
                                       smoother=SMOOTHERS[smname])
    estimate = ogamg.estimate_emax_cg if eig_ksp == 1 else ogamg.estimate_emax
    with A, ksp:
        check_refreshed(h0, h1, aa1, exact_ref=True)
        for l in range(len(h1[0]) - 1):
            ai, aj, aa, n = h1[2][l]
            Al = sp.csr_matrix((aa, aj, ai), shape=(n, n))
            d = ogamg.first_diagonal(Al)
            lam = estimate(Al, 1.0 / np.where(d == 0.0, 1.0, d), 10)
            ty, its, emin, emax = ksp.mg_smoother(l)
            assert (ty, its) == ("chebyshev", SMOOTHERS[smname]["its"])
            assert_bits([emin, emax], [sm.cheby_lo * lam, sm.cheby_hi * lam], f"level {l} Chebyshev bounds")
            assert (emin, emax) != before[l][2:]


# 2 ---- identity and scaling
def vcycles_and_solve(pkg, ksp, csr, N, tol):
    """pc_apply on the five V-cycle columns and one solve: (Z columns, x, its, reason, history)."""
    m = len(csr[0]) - 1
    rhs, _ = pkg.poisson_vectors(N)
    cols = named_columns(m, rhs, pkg.splitmix_uniform(m, 42))
    zs = []
    for name in VCYCLE_COLUMNS:
        r = torch.tensor(cols[name]).cuda()
        z = torch.full((m,), SENTINEL, dtype=torch.float64, device="cuda")
        ksp.pc_apply(r, z)
        torch.cuda.synchronize()
        zs.append(z.cpu().numpy())
    b = torch.from_numpy(rhs).cuda()
    x = torch.full((m,), SENTINEL, dtype=torch.float64, device="cuda")
    ksp.solve(b, x)
    torch.cuda.synchronize()
    return zs, x.cpu().numpy(), ksp.its, ksp.reason, ksp.history().copy()


def assert_nan_bits(got, want, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert_bits(got[~nan], want[~nan], what)


@pytest.mark.parametrize("smname", ["default", "chebyshev2"])
@pytest.mark.parametrize("plan", ["templates", "csr"])
def test_refresh_to_the_same_values_changes_no_bit(pkg, plan, smname):
    N = 12
    csr, _ = operand(pkg, N)
    tol = dict(rtol=1e-10, atol=1e-50, max_it=200)
    A, ksp = make(pkg, csr, plan, smoother=SMOOTHERS[smname], reuse_interpolation=True, **tol)
    with A, ksp:
        ksp.set_up()
        h0 = hierarchy(ksp)
        first = vcycles_and_solve(pkg, ksp, csr, N, tol)
        A.update_values(csr[2])
        ksp.set_up()
        assert ksp.setup_counts()[:2] == (1, 1)
        assert_same_hierarchy(hierarchy(ksp), h0)
        again = vcycles_and_solve(pkg, ksp, csr, N, tol)
        for z0, z1, name in zip(first[0], again[0], VCYCLE_COLUMNS):
            assert_nan_bits(z1, z0, f"pc_apply on {name}")
        assert again[2:4] == first[2:4] and first[3] > 0
        assert_bits(again[1], first[1], "x")
        assert_bits(again[4], first[4], "history")


@pytest.mark.parametrize("smname", ["default", "richardson2-scale0.9", "chebyshev1", "chebyshev2"])
def test_refresh_to_four_times_the_values_scales_exactly(pkg, smname):
    """Scaling by a power of two commutes with every rounding on the path:
    every A_l is exactly 4 x the old, the V-cycle gives exactly z / 4, the
    solve exactly x / 4 with the same iterations and history / 4. A refresh
    step that still held an old value would show as a bit difference."""
    N = 12
    csr, _ = operand(pkg, N)
    tol = dict(rtol=1e-10, atol=1e-50, max_it=200)
    A, ksp = make(pkg, csr, "csr", smoother=SMOOTHERS[smname], reuse_interpolation=True, **tol)
    with A, ksp:
        ksp.set_up()
        h0 = hierarchy(ksp)
        first = vcycles_and_solve(pkg, ksp, csr, N, tol)
        A.update_values(4.0 * csr[2])
        ksp.set_up()
        assert ksp.setup_counts()[:2] == (1, 1)
        h1 = hierarchy(ksp)
        for a0, a1 in zip(h0[2], h1[2]):
            assert np.array_equal(a0[0], a1[0]) and np.array_equal(a0[1], a1[1])
            assert_bits(a1[2], 4.0 * a0[2], "A_l = 4 x the old")
        for p0, p1 in zip(h0[3], h1[3]):
            assert same_bits(p0[:3], p1[:3])
        again = vcycles_and_solve(pkg, ksp, csr, N, tol)
        for z0, z1, name in zip(first[0], again[0], VCYCLE_COLUMNS):
            assert_nan_bits(z1, z0 / 4.0, f"pc_apply on {name}")
        assert again[2:4] == first[2:4] and first[3] > 0
        assert_bits(again[1], first[1] / 4.0, "x / 4")
        assert_bits(again[4], first[4] / 4.0, "history / 4")


# 3 ---- flag off, and structure
def test_flag_off_rebuilds_and_flag_on_keeps_the_interpolation(pkg):
    N = 12
    csr, _ = operand(pkg, N)
    aa1 = sas(csr)
    m = len(csr[0]) - 1
    # the oracle says the prolongators of A and A' differ
    lv0 = ogamg.build(sp.csr_matrix((csr[2], csr[1], csr[0]), shape=(m, m)))
    lv1 = ogamg.build(sp.csr_matrix((aa1, csr[1], csr[0]), shape=(m, m)))
    must_differ = len(lv0) != len(lv1) or lv0[0]["P"].shape != lv1[0]["P"].shape or \
        not np.array_equal(lv0[0]["P"].data.view(np.uint64), lv1[0]["P"].data.view(np.uint64))
    assert must_differ
    with pkg.SeqAIJHIP(csr[0], csr[1], aa1) as Af, K_().KSPCG(Af, pc="gamg") as fresh:
        fresh.set_up()
        assert fresh.setup_counts()[:2] == (1, 0) and fresh.reuse_interpolation is False
        hf = hierarchy(fresh)
    A, ksp = make(pkg, csr, "templates")  # the default: flag off
    with A, ksp:
        assert ksp.reuse_interpolation is False
        ksp.set_up()
        A.update_values(aa1)
        ksp.set_up()
        assert ksp.setup_counts()[:2] == (2, 0)  # today's behaviour: two full set-ups
        assert_same_hierarchy(hierarchy(ksp), hf)
    A, ksp, h0, h1, _ = refresh_case(pkg, N, "default", "templates")
    with A, ksp:
        same = len(h1[3]) == len(hf[3]) and all(p[3] == q[3] and same_bits(p[:3], q[:3]) for p, q in zip(h1[3], hf[3]))
        assert not same, "the refreshed P_l must be the first set-up's, not a fresh handle's"
        # the flag set on a handle that is already set up: the next change refreshes
        ksp.reuse_interpolation = False
        A.update_values(csr[2])
        ksp.set_up()
        assert ksp.setup_counts()[:2] == (2, 1)
        ksp.reuse_interpolation = True
        A.update_values(aa1)
        ksp.set_up()
        assert ksp.setup_counts()[:2] == (2, 2)
        check_refreshed(hierarchy(ksp), hierarchy(ksp), aa1, exact_ref=True)


def test_new_structure_takes_the_full_setup(pkg):
    """assembly_end with one entry removed (and its mirror): a new structure,
    so a full set-up although the flag is on; a re-plan by set_option is not."""
    N = 8
    csr, _ = operand(pkg, N)
    ai, aj, aa = csr
    A, ksp = make(pkg, csr, "templates", reuse_interpolation=True)
    with A, ksp:
        ksp.set_up()
        A.set_option("row_templates", 0)  # the plan moves, the structure does not
        ksp.set_up()
        assert ksp.setup_counts()[:2] == (1, 1)
        rows = rows_of(ai)
        k = int(np.flatnonzero((rows == 5) & (aj != 5))[0])
        j = int(aj[k])
        drop = np.zeros(len(aj), bool)
        drop[k] = True
        drop[np.flatnonzero((rows == j) & (aj == 5))] = True
        ai2 = np.concatenate(([0], np.cumsum(np.bincount(rows[~drop], minlength=len(ai) - 1)))).astype(np.int32)
        A.assembly_end(ai2, aj[~drop], aa[~drop])
        ksp.set_up()
        assert ksp.setup_counts()[:2] == (2, 1)
        with pkg.SeqAIJHIP(ai2, aj[~drop], aa[~drop], row_templates=0) as Af, K_().KSPCG(Af, pc="gamg") as fresh:
            fresh.set_up()
            assert_same_hierarchy(hierarchy(ksp), hierarchy(fresh))
        # a PC that is not GAMG ignores the flag
    with pkg.SeqAIJHIP(*csr) as Aj, K_().KSPCG(Aj, pc="jacobi", reuse_interpolation=True) as kj:
        kj.set_up()
        Aj.update_values(2.0 * aa)
        kj.set_up()
        assert kj.setup_counts()[:2] == (2, 0)


# 4 ---- the V-cycle and solves after a refresh
@pytest.mark.parametrize("smname", ["default", "chebyshev2"])
@pytest.mark.parametrize("plan", ["templates", "csr"])
@pytest.mark.parametrize("N", [12, 24])
def test_vcycle_and_solves_after_a_refresh(pkg, N, plan, smname):
    """Against a SCALAR-kernel handle taken through the same sequence, against
    ogamg.vcycle on the oracle levels (Richardson(1): what the oracle's cycle
    smooths with), and mat_solve against the single solves."""
    csr, _ = operand(pkg, N)
    m = len(csr[0]) - 1
    tol = dict(rtol=1e-10, atol=1e-50, max_it=200)
    kw = dict(smoother=SMOOTHERS[smname], mat_vcycle=4, **tol)
    R, kr, _, hr, aa1 = refresh_case(pkg, N, "default", "generic", **kw)
    A, ksp, h0, h1, _ = refresh_case(pkg, N, "default", plan, **kw)
    with R, kr, A, ksp:
        assert kr.fused is False
        assert_same_hierarchy(h1, hr)
        exact = longest_row(h1) <= 128
        print(f"{N}^3 {plan} {smname}: levels {h1[0]}, {'bitwise' if exact else 'bars'}")
        blocks = [ksp.pc_levels()[2], ksp.setup_counts()]
        csr1 = (csr[0], csr[1], aa1)
        ref = vcycles_and_solve(pkg, kr, csr1, N, tol)
        got = vcycles_and_solve(pkg, ksp, csr1, N, tol)
        for z0, z1, name in zip(ref[0], got[0], VCYCLE_COLUMNS):
            assert_column(z1, z0, exact, f"pc_apply on {name}")
        # the handle's own single solve sums CG's dots in its fused launches' block order, the
        # SCALAR handle's in passes of their own: not the same bits by the library's contract
        # (include/aijhip_ksp.h, aijhip_ksp_mat_solve), so the bar is the one tests/test_gamg.py
        # holds CG + GAMG to across summation orders (:165-170); the bit-for-bit single solves
        # are mat_solve's columns below
        assert got[3] == ref[3] > 0 and abs(got[2] - ref[2]) <= 1, (got[2:4], ref[2:4])
        k = min(10, len(got[4]), len(ref[4]))
        np.testing.assert_allclose(got[4][:k], ref[4][:k], rtol=1e-7)
        assert np.linalg.norm(got[1] - ref[1]) <= 1e-8 * np.linalg.norm(ref[1])
        if smname == "default":
            # the oracle's V-cycle on (A_l' by the chain, kept P_l): the bars a V-cycle's Z is
            # held to across summation orders (rtol 1e-10, atol 1e-12 max|z|)
            chain = oracle_chain(csr1, h1[3], exact_ref=False)
            levels = []
            for l, (ci, cj, ca) in enumerate(chain):
                n = len(ci) - 1
                L = dict(A=sp.csr_matrix((ca, cj, ci), shape=(n, n)))
                if l < len(h1[3]):
                    pi, pj, pa, nc = h1[3][l]
                    L["P"] = sp.csr_matrix((pa, pj, pi), shape=(n, nc))
                levels.append(L)
            rhs, _ = pkg.poisson_vectors(N)
            zo = ogamg.vcycle(levels, rhs)
            np.testing.assert_allclose(got[0][0], zo, rtol=1e-10, atol=1e-12 * np.abs(zo).max())
        # mat_solve on the refreshed handle, column by column the refreshed single solves
        rhs, _ = pkg.poisson_vectors(N)
        cols = named_columns(m, rhs, pkg.splitmix_uniform(m, 42))
        names = ("rhs", "splitmix", "spike", "small_rhs")
        B = torch.tensor(np.stack([cols[n] for n in names], axis=1)).cuda()
        X = torch.full((m, 4), SENTINEL, dtype=torch.float64, device="cuda")
        reserve = ksp.mat_vcycle_reserve()  # (refresh_case asserted: the first set-up's)
        ksp.mat_solve(B, X)
        torch.cuda.synchronize()
        res = ksp.mat_results()
        Xh = X.cpu().numpy()
        for j, name in enumerate(names):
            b = torch.tensor(cols[name]).cuda()
            x = torch.full((m,), SENTINEL, dtype=torch.float64, device="cuda")
            kr.solve(b, x)
            torch.cuda.synchronize()
            assert (res[j][0], res[j][1]) == (kr.its, kr.reason) and kr.reason > 0, (name, res[j], kr.its, kr.reason)
            assert_column(Xh[:, j], x.cpu().numpy(), exact, f"mat_solve column {name}")
        # nothing of the hierarchy or the multi-column reserve was rebuilt for it
        assert [ksp.pc_levels()[2], ksp.setup_counts()] == blocks and ksp.setup_counts()[:2] == (1, 1)
        assert_reserve_kept(ksp, reserve, "mat_solve after the refresh")


@pytest.mark.parametrize("smname", ["default", "chebyshev2"])
def test_refreshed_hierarchy_still_converges(pkg, smname):
    """Against a handle freshly set up on A' with the same tolerances: a
    positive reason and a true residual at most 10 x the fresh handle's (both
    stop on the same preconditioned-norm test; the margin covers the other
    preconditioner). The iteration counts are printed, not bounded."""
    N = 24
    csr, _ = operand(pkg, N)
    m = len(csr[0]) - 1
    tol = dict(rtol=1e-10, atol=1e-50, max_it=500)
    rhs, _ = pkg.poisson_vectors(N)
    b = torch.from_numpy(rhs).cuda()
    A, ksp, h0, h1, aa1 = refresh_case(pkg, N, "default", "templates", smoother=SMOOTHERS[smname], **tol)
    A1 = sp.csr_matrix((aa1, csr[1], csr[0]), shape=(m, m))
    with A, ksp, pkg.SeqAIJHIP(csr[0], csr[1], aa1) as Af, \
            K_().KSPCG(Af, pc="gamg", smoother=SMOOTHERS[smname], **tol) as fresh:
        out = []
        for k in (ksp, fresh):
            x = torch.zeros_like(b)
            k.solve(b, x)
            torch.cuda.synchronize()
            out.append((k.its, k.reason, float(np.linalg.norm(rhs - A1 @ x.cpu().numpy()))))
        print(f"{smname}: refreshed its {out[0][0]} residual {out[0][2]:.3e}; fresh its {out[1][0]} residual {out[1][2]:.3e}")
        assert out[0][1] > 0 and out[1][1] > 0, out
        assert out[0][2] <= 10.0 * out[1][2], out


# 5 ---- other rows (last: the stand-ins' set-ups are the largest here)
@pytest.mark.parametrize("plan", ["templates", "csr", "generic"])
@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("key", ["fem_hex", "skewed"])
def test_refresh_standin_hierarchy(pkg, key, where, plan):
    A, ksp, h0, h1, aa1 = refresh_case(pkg, key, where, plan)
    with A, ksp:
        print(f"{key} {where} {plan}: levels {h1[0]}, nnz {h1[1]}, longest row {longest_row(h1)}")
        assert len(h1[0]) >= 2
        check_refreshed(h0, h1, aa1, exact_ref=False)
