"""The solver ops on row templates beyond the 7-point Poisson operand.

CG and the V-cycle run on the row-template launches (csrc/aijhip_kernels.hip),
which choose a kernel by the plan: templates of at most 7 entries take the
pipelined kernel with 7 gather slots, of 8 entries the one with 8, longer
ones the 2-rows-per-lane kernel; with a diagonal in every template the dot,
and the post-smoothing's t[r], come from the gathered diagonal slot, else
from a load. The Poisson operand reaches one corner of that (7 entries, a
diagonal everywhere, in slots 0-3). The operands here reach the others:

  paired7     7-point + one coupling two columns away: 8 entries, diagonal
              slots 0-4, 3 row blocks (a grid below 8) and 22 (XCD chunks of
              2-3 blocks: workgroups with an odd count sum their last twice)
  no-diag     paired7 with three rows and columns removed: a template of
              no entries, so no diagonal slot and the loading op forms
  hub_chain   tridiagonal with a few rows reaching back 5-7 columns: the
              diagonal in slots 5, 6 and 7 of 7- and 8-entry rows
  box9        the 9-point box stencil: 9 entries, the 2-rows-per-lane kernel
              and its reduction over 8 wave sums

Every solve is compared bit for bit across the aj, row-pattern and
row-template layouts and with AIJHIP_KSP_EXPLICIT_Z=1 (the stored Z and
D^-1 against the per-template ones), and against the CPU oracle at the bars
of tests/test_ksp.py and tests/test_gamg.py."""
import importlib

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import gamg as ogamg
from oracle import ksp_cg
from test_row_patterns_gpu import assert_bits, box_stencil_csr

gpu = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL = dict(rtol=1e-14, atol=1e-12, max_it=10000)  # configs/cg_gamg.info
LAYOUTS = {"aj": dict(row_patterns=0, row_templates=0, column_codes=0),
           "patterns": dict(row_patterns=1, row_templates=0),
           "templates": dict(row_patterns=1, row_templates=1)}


def _csr(A):
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)


def paired7(nz, ny, nx, c=0.5):
    """7-point Laplacian (6 + c on the diagonal, -1 off it) plus a symmetric
    coupling -c between (.., ix) and (.., ix + 2) where ix % 4 < 2: every
    point has exactly one partner when nx % 4 == 0, interior rows 8 entries."""
    idx = np.arange(nz * ny * nx).reshape(nz, ny, nx)
    r = [idx.ravel()]
    c_ = [idx.ravel()]
    v = [np.full(idx.size, 6.0 + c)]
    for ax in range(3):
        lo = idx.take(np.arange(idx.shape[ax] - 1), axis=ax).ravel()
        hi = idx.take(np.arange(1, idx.shape[ax]), axis=ax).ravel()
        r += [lo, hi]
        c_ += [hi, lo]
        v += [np.full(lo.size, -1.0)] * 2
    ix = np.arange(nx)
    left = ix[(ix % 4 < 2) & (ix + 2 < nx)]
    lo, hi = idx[:, :, left].ravel(), idx[:, :, left + 2].ravel()
    r += [lo, hi]
    c_ += [hi, lo]
    v += [np.full(lo.size, -c)] * 2
    m = idx.size
    return _csr(sp.coo_matrix((np.concatenate(v), (np.concatenate(r), np.concatenate(c_))), shape=(m, m)))


def without_rows(csr, rows):
    """The operand with these rows and their columns removed (empty rows)."""
    ai, aj, aa = csr
    m = len(ai) - 1
    keep = np.ones(m)
    keep[list(rows)] = 0.0
    D = sp.diags(keep)
    A = sp.csr_matrix(D @ sp.csr_matrix((aa, aj, ai), shape=(m, m)) @ D)
    A.eliminate_zeros()
    return _csr(A)


def hub_chain(m, hubs):
    """Tridiagonal (-1, 2.5, -1); hub row h of (h, k) in hubs also couples,
    with -0.25, to rows h - 2 .. h - k, 0.25 per coupling added to both
    diagonals (diagonally dominant: the smallest eigenvalue stays 0.5)."""
    A = sp.diags([np.full(m - 1, -1.0), np.full(m, 2.5), np.full(m - 1, -1.0)], [-1, 0, 1], format="lil")
    for h, k in hubs:
        for j in range(2, k + 1):
            A[h, h - j] = A[h - j, h] = -0.25
            A[h, h] += 0.25
            A[h - j, h - j] += 0.25
    return _csr(A)


def _hubs(m):
    """Inner hubs every 41 rows, reaching back 5 and 6 rows in turn (7 and 8
    entries, the diagonal in slots 5 and 6), and the last row reaching back
    7 (8 entries, no upper neighbour: slot 7)."""
    inner = [(h, 5 + i % 2) for i, h in enumerate(range(20, m - 20, 41))]
    return inner + [(m - 1, 7)]


EMPTY_ROWS = (5, 700, 1079)
# name -> (builder, longest row, a diagonal in every row)
OPERANDS = {
    "paired7-3blocks": (lambda: paired7(9, 10, 12), 8, True),
    "paired7-22blocks": (lambda: paired7(33, 20, 17), 8, True),
    "paired7-empty-rows": (lambda: without_rows(paired7(9, 10, 12), EMPTY_ROWS), 8, False),
    "hub-chain-1500": (lambda: hub_chain(1500, _hubs(1500)), 8, True),
    "hub-chain-7000": (lambda: hub_chain(7000, _hubs(7000)), 8, True),
    "box9-40x37": (lambda: box_stencil_csr(1, 40, 37), 9, True),
    "box9-90x83": (lambda: box_stencil_csr(1, 90, 83), 9, True),
}
PIPELINED = [n for n, o in OPERANDS.items() if o[1] <= 8]
_cache = {}


def operand(name):
    """(ai, aj, aa, b): b uniform in [-1, 1), 0 on the empty rows."""
    if ("op", name) not in _cache:
        ai, aj, aa = OPERANDS[name][0]()
        m = len(ai) - 1
        b = np.random.default_rng(len(name) + m).uniform(-1, 1, m)
        b[np.diff(ai) == 0] = 0.0
        _cache["op", name] = (ai, aj, aa, b)
    return _cache["op", name]


def diagonal_slots(ai, aj):
    """The positions of the diagonal within the rows that store one."""
    rows = np.repeat(np.arange(len(ai) - 1), np.diff(ai))
    k = np.flatnonzero(aj == rows)
    return set((k - ai[rows[k]]).tolist()), len(k)


def check_branch(name):
    """Conditions on the INPUT, before any GPU work: the operand reaches the
    launch it is here for (row length, diagonals, and what the planner asks
    of a template operand: mean row <= 16, at most 256 distinct rows)."""
    ai, aj, aa, _ = operand(name)
    _, maxlen, all_diag = OPERANDS[name]
    m = len(ai) - 1
    lens = np.diff(ai)
    assert lens.max() == maxlen
    assert (diagonal_slots(ai, aj)[1] == m) == all_diag
    assert lens.mean() <= 16
    rows = np.repeat(np.arange(m), lens)
    temps = {tuple(aj[ai[i]:ai[i + 1]] - rows[ai[i]:ai[i + 1]]) + tuple(aa[ai[i]:ai[i + 1]].view(np.uint64))
             for i in range(m)}
    assert len(temps) <= 256
    assert len(temps) + sum(len(t) // 2 for t in temps) <= 1024


@pytest.mark.parametrize("name", list(OPERANDS))
def test_operand_reaches_its_branch(name):
    check_branch(name)


def test_family_reaches_every_diagonal_slot():
    """The operands of the pipelined launch put the diagonal in each of its
    8 slots (the Poisson operand: 0-3 only)."""
    slots = set()
    for name in PIPELINED:
        ai, aj, _, _ = operand(name)
        slots |= diagonal_slots(ai, aj)[0]
    assert slots == set(range(8))


@pytest.fixture(autouse=True)
def _plain_env(monkeypatch):
    monkeypatch.delenv("AIJHIP_KSP_EXPLICIT_Z", raising=False)
    monkeypatch.delenv("AIJHIP_MG_UNFUSED", raising=False)


def gpu_solve(pkg, name, pc, layout="templates", norm="preconditioned", expect_fused=True):
    """(its, reason, history, x, level rows) of one solve from x = 0. The
    environment is read at set-up, so a caller sets it before this."""
    K = importlib.import_module("petsc-openacc_amd.ksp")
    ai, aj, aa, rhs = operand(name)
    dev = torch.device("cuda:0")
    b = torch.from_numpy(rhs).to(dev)
    with pkg.SeqAIJHIP(ai, aj, aa, **LAYOUTS[layout]) as A:
        info = A.info()
        assert info["row_templates"] == (layout == "templates")
        assert (info["row_patterns"] > 0) == (layout != "aj")
        x = torch.zeros_like(b)
        with K.KSPCG(A, pc=pc, norm=norm, **TOL) as ksp:
            ksp.set_up()
            ksp.solve(b, x)
            torch.cuda.synchronize()
            assert ksp.fused == expect_fused
            rows = ksp.pc_levels()[0] if pc == "gamg" else None
            return ksp.its, ksp.reason, np.array(ksp.history()), x.cpu().numpy(), rows


def base_solve(pkg, name, pc, layout="templates", norm="preconditioned"):
    """gpu_solve in the default environment, once per case."""
    key = ("gpu", name, pc, layout, norm)
    if key not in _cache:
        _cache[key] = gpu_solve(pkg, name, pc, layout, norm)
    return _cache[key]


def assert_same_solve(a, b):
    assert (a[0], a[1]) == (b[0], b[1])
    assert len(a[2]) == len(b[2])
    assert_bits(a[2], b[2])
    assert_bits(a[3], b[3])


def oracle_solve(name, pc, norm="preconditioned"):
    key = ("oracle", name, pc, norm)
    if key not in _cache:
        ai, aj, aa, rhs = operand(name)
        m = len(ai) - 1
        rows = None
        apply_pc = pc
        if pc == "gamg":
            if ("levels", name) not in _cache:
                _cache["levels", name] = ogamg.build(sp.csr_matrix((aa, aj, ai), shape=(m, m)), coarse_eq_limit=50)
            levels = _cache["levels", name]
            rows = [L["A"].shape[0] for L in levels]
            apply_pc = lambda r: ogamg.vcycle(levels, r)  # noqa: E731
        Asp = sp.csr_matrix((aa, aj, ai), shape=(m, m))
        _cache[key] = ksp_cg.cg(ai, aj, aa, rhs, pc=apply_pc, norm=norm, matmult=lambda v: Asp @ v, **TOL) + (rows,)
    return _cache[key]


def assert_matches_oracle(got, ref, pc):
    """tests/test_ksp.py:72-80 (Jacobi) and tests/test_gamg.py:164-170."""
    its, reason, h, x, rows = got
    xo, its_o, reason_o, hist_o, rows_o = ref
    assert reason == reason_o, (reason, reason_o)
    assert abs(its - its_o) <= 1, (its, its_o)
    n, rtol, xtol = (30, 1e-8, 1e-9) if pc == "jacobi" else (10, 1e-7, 1e-8)
    k = min(n, len(h), len(hist_o))
    np.testing.assert_allclose(h[:k], hist_o[:k], rtol=rtol)
    assert np.linalg.norm(x - xo) <= xtol * np.linalg.norm(xo)
    assert rows == rows_o


@gpu
@pytest.mark.parametrize("pc", ["jacobi", "gamg"])
@pytest.mark.parametrize("name", list(OPERANDS))
def test_solve_bitwise_across_layouts(pkg, name, pc):
    """Iterations, reason, residual history and solution of the fused solve
    equal bit for bit with aj, with row patterns and with row templates."""
    check_branch(name)
    ref = base_solve(pkg, name, pc, "aj")
    for layout in ("patterns", "templates"):
        assert_same_solve(base_solve(pkg, name, pc, layout), ref)


@gpu
@pytest.mark.parametrize("pc", ["jacobi", "gamg"])
@pytest.mark.parametrize("name", list(OPERANDS))
def test_implicit_z_gives_the_stored_z_bits(pkg, monkeypatch, name, pc):
    """AIJHIP_KSP_EXPLICIT_Z=1 (the stored Z and per-row D^-1) against the
    default on templates (Z formed where it is read, D^-1 per template)."""
    check_branch(name)
    ref = base_solve(pkg, name, pc)
    monkeypatch.setenv("AIJHIP_KSP_EXPLICIT_Z", "1")
    assert_same_solve(gpu_solve(pkg, name, pc), ref)


@gpu
@pytest.mark.parametrize("pc", ["jacobi", "gamg"])
@pytest.mark.parametrize("name", list(OPERANDS))
def test_solve_matches_oracle(pkg, name, pc):
    """The template solve against KSPSolve_CG's restatement (with the
    oracle's V-cycle on the oracle's hierarchy for GAMG; the empty-row
    operand included: its empty rows join no aggregate)."""
    check_branch(name)
    assert_matches_oracle(base_solve(pkg, name, pc), oracle_solve(name, pc), pc)


@gpu
@pytest.mark.parametrize("name", ["paired7-3blocks", "box9-40x37"])
def test_unpreconditioned_norm_matches_oracle(pkg, name):
    """CG + Jacobi testing r.r instead of z.z: another dot of the fused
    update, on one operand per template kernel; the three layouts bitwise."""
    check_branch(name)
    got = base_solve(pkg, name, "jacobi", norm="unpreconditioned")
    assert_matches_oracle(got, oracle_solve(name, "jacobi", "unpreconditioned"), "jacobi")
    for layout in ("aj", "patterns"):
        assert_same_solve(base_solve(pkg, name, "jacobi", layout, "unpreconditioned"), got)


@gpu
@pytest.mark.parametrize("name", ["paired7-3blocks", "box9-40x37"])
def test_vcycle_fused_against_unfused(pkg, monkeypatch, name):
    """AIJHIP_MG_UNFUSED=1 (separate smoother, residual and vector passes) at
    test_gpu_vcycle_fused_smoothers_bitwise's bars: the same iterations, the
    history within 1e-12 — one operand per template kernel."""
    check_branch(name)
    its, _, h, x, _ = base_solve(pkg, name, "gamg")
    monkeypatch.setenv("AIJHIP_MG_UNFUSED", "1")
    its_u, _, h_u, x_u, _ = gpu_solve(pkg, name, "gamg")
    assert its_u == its
    np.testing.assert_allclose(h_u, h, rtol=1e-12, atol=1e-15 * h[0])
    np.testing.assert_allclose(x_u, x, rtol=1e-10, atol=1e-12 * np.abs(x).max())
