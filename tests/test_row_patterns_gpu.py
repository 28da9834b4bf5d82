"""Row patterns (AIJHIP_OPT_ROW_PATTERNS) and row templates
(AIJHIP_OPT_ROW_TEMPLATES: the patterns with their values, for a constant-
coefficient stencil; neither aj nor aa read): for short-row operands whose rows
follow at most 256 distinct column - row offset lists (a stencil), the STREAM
row blocks read no column per entry — a pattern id per row, the lists staged
in LDS, x gathered by one lane per row. aa and the summation (s = seed, then
s += aa[k] * x[col] in storage order) are the plain kernel's, so every result
must be BIT-IDENTICAL to the aj layout and to the oracle (the PETSc row loop,
/root/reference/src/openacc-step1/MatMult_SeqAIJ.patch:22-31)."""
import importlib

import numpy as np
import pytest

from conftest import GOLDEN_NAMES, golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev(pkg):
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def assert_bits(a, b, mask=None):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if mask is not None:
        a, b = a[mask], b[mask]
    bad = np.nonzero(a.view(np.uint64) != b.view(np.uint64))[0]
    assert bad.size == 0, f"{bad.size}/{a.size} entries differ bitwise; first {bad[:4]}: {a[bad[:4]]} vs {b[bad[:4]]}"


def products(A, x, z, dev):
    xd, zd = to_dev(x, dev), to_dev(z, dev)
    y = torch.full((A.m,), np.nan, dtype=torch.float64, device=dev)
    w = torch.full((A.m,), np.nan, dtype=torch.float64, device=dev)
    A.mult(xd, y)
    A.mult_add(xd, zd, w)
    torch.cuda.synchronize()
    return y.cpu().numpy(), w.cpu().numpy()


@pytest.mark.parametrize("dims", [(37, 37, 37), (20, 17, 13), (1, 9, 40), (300, 2, 3)])
def test_poisson_patterns_bitwise(pkg, dev, coracle, dims):
    """7-point Poisson with the reference point (helper.cpp:161-279), cubes,
    boxes and thin grids: the automatic layout takes row templates (the
    distinct rows, offsets and values: interior, faces, edges, corners, the
    reference rows; AIJHIP_OPT_ROW_TEMPLATES), or with templates off row
    patterns (the distinct offset lists). MatMult and MatMultAdd equal the
    oracle and the aj layout bit for bit in all three, also after new values:
    values that no longer fit the templates re-plan to the patterns, values
    that do keep them."""
    ai, aj, aa = pkg.poisson_csr(*dims)
    m = len(ai) - 1
    x, z = pkg.splitmix_uniform(m, 42), pkg.splitmix_uniform(m, 7)
    rows = np.repeat(np.arange(m), np.diff(ai))
    lists = {tuple(aj[ai[i]:ai[i + 1]] - rows[ai[i]:ai[i + 1]]) for i in range(m)}  # the distinct offset lists
    temps = {tuple(aj[ai[i]:ai[i + 1]] - rows[ai[i]:ai[i + 1]]) + tuple(aa[ai[i]:ai[i + 1]].view(np.uint64))
             for i in range(m)}  # the distinct rows
    with pkg.SeqAIJHIP(ai, aj, aa) as A:
        info = A.info()
        assert (info["row_templates"], info["row_patterns"], info["column_codes"]) == (1, len(temps), 0)
        assert info["mult_layout_bytes"] == m + 12 * (len(temps) + sum(len(t) // 2 for t in temps)) + 16 * m
        yt, wt = products(A, x, z, dev)
        assert_bits(yt, coracle.matmult(ai, aj, aa, x, omp=True))
        A.set_option("row_templates", 0)
        assert (A.info()["row_templates"], A.info()["row_patterns"]) == (0, len(lists))
        y1, w1 = products(A, x, z, dev)
        assert_bits(yt, y1)
        assert_bits(wt, w1)
        A.set_option("row_patterns", 0)
        A.set_option("column_codes", 0)
        assert A.info()["row_patterns"] == 0
        y0, w0 = products(A, x, z, dev)
        assert_bits(y1, y0)
        assert_bits(w1, w0)
        A.set_option("row_patterns", -1)
        A.set_option("row_templates", -1)
        assert A.info()["row_templates"] == 1
        A.update_values(2.0 * aa)  # still one template per distinct row
        assert A.info()["row_templates"] == 1
        y3, _ = products(A, x, z, dev)
        assert_bits(y3, coracle.matmult(ai, aj, 2.0 * aa, x, omp=True))
        aa2 = np.random.default_rng(5).uniform(-1, 1, len(aa))
        A.update_values(aa2)  # the patterns do not depend on the values; the templates do
        assert (A.info()["row_templates"], A.info()["row_patterns"]) == (0, len(lists))
        y2, _ = products(A, x, z, dev)
        assert_bits(y2, coracle.matmult(ai, aj, aa2, x, omp=True))


def box_stencil_csr(nz, ny, nx):
    """Constant-coefficient box stencil (27 points in 3-D, 9 with nz = 1) on
    an nz x ny x nx grid: the point count less one on the diagonal, -1 off
    it; rows of up to 27 (9) entries."""
    idx = np.arange(nz * ny * nx).reshape(nz, ny, nx)
    rows, cols, vals = [], [], []
    dzs = (-1, 0, 1) if nz > 1 else (0,)
    npts = 9 * len(dzs)
    for dz in dzs:
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                def sl(d, n):
                    return slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d))
                (sz, tz), (sy, ty), (sx, tx) = sl(dz, nz), sl(dy, ny), sl(dx, nx)
                src, dst = idx[sz, sy, sx], idx[tz, ty, tx]
                rows.append(src.ravel())
                cols.append(dst.ravel())
                vals.append(np.full(src.size, npts - 1.0 if (dz, dy, dx) == (0, 0, 0) else -1.0))
    r, c, v = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    o = np.lexsort((c, r))
    r, c, v = r[o], c[o], v[o]
    ai = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=nz * ny * nx))]).astype(np.int32)
    return ai, c.astype(np.int32), v


@pytest.mark.parametrize("dims", [(1, 40, 37), (1, 700, 650)])
def test_templates_longer_than_the_fast_slots(pkg, dev, coracle, dims):
    """Row templates of 9 entries (a 2-D 9-point stencil; mean row <= 16, so
    templates apply): more than the pipelined kernel's 8 fast slots, so the
    launch takes the 2-rows-per-lane template kernel; MatMult / MatMultAdd
    bitwise the oracle's and the row patterns' (templates off)."""
    ai, aj, aa = box_stencil_csr(*dims)
    m = len(ai) - 1
    assert np.diff(ai).max() == 9
    x, z = pkg.splitmix_uniform(m, 3), pkg.splitmix_uniform(m, 4)
    with pkg.SeqAIJHIP(ai, aj, aa) as A:
        assert A.info()["row_templates"] == 1
        yt, wt = products(A, x, z, dev)
        assert_bits(yt, coracle.matmult(ai, aj, aa, x, omp=True))
        A.set_option("row_templates", 0)
        assert A.info()["row_patterns"] > 0
        y1, w1 = products(A, x, z, dev)
        assert_bits(yt, y1)
        assert_bits(wt, w1)


@pytest.mark.parametrize("m,n", [(119, 4), (250, 17), (1537, None), (70001, None)])
def test_templates_inplace_mult_add(pkg, dev, coracle, m, n):
    """In-place MatMultAdd (w = z, PCMG's x = x + P x_c) on row templates: a
    coarse prolongator's shape (m x n, n < m, every row its own template) and
    banded operators of one to 137 row blocks (a few value patterns). A lane
    past a block's rows and the re-summed last block of a workgroup must not
    store — another wave may already have updated that row, which an
    in-place add reads as its seed. w equals z + A x bit for bit."""
    rng = np.random.default_rng(m)
    if n is not None:
        rows = [np.unique(rng.integers(0, n, rng.integers(1, 4))) for _ in range(m)]
        vals = [rng.uniform(-1, 1, len(c)) for c in rows]
    else:
        n = m
        rows = [np.arange(max(0, i - 1), min(m, i + 2)) for i in range(m)]
        pick = rng.integers(0, 3, m)
        vals = [np.array([0.5, -1.0, 2.0, 0.25])[(pick[i] + np.arange(len(c))) % 4] for i, c in enumerate(rows)]
    ai = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int32)
    aj = np.concatenate(rows).astype(np.int32)
    aa = np.concatenate(vals)
    x, z = rng.uniform(-1, 1, n), rng.uniform(-1, 1, m)
    ref = coracle.matmult_add(ai, aj, aa, x, z)
    with pkg.SeqAIJHIP(ai, aj, aa, ncols=n, row_patterns=1) as A:
        assert A.info()["row_templates"] == 1
        xd, zd = to_dev(x, dev), to_dev(z, dev)
        w = zd.clone()
        A.mult_add(xd, w, w)
        w2 = torch.full_like(zd, np.nan)
        A.mult_add(xd, zd, w2)
        torch.cuda.synchronize()
        assert_bits(w.cpu().numpy(), ref)
        assert_bits(w2.cpu().numpy(), ref)


def test_templates_cg_dots_match_csr_on_odd_block_counts(pkg, dev):
    """CG + Jacobi on operands whose persistent template grid leaves some
    workgroups an odd number of row blocks (the last one summed twice) and
    blocks shorter than 512 rows: the residual history and solution equal
    the CSR layout's bit for bit (the fused SpMV + p.w partials per block)."""
    K = importlib.import_module("petsc-openacc_amd.ksp")
    for dims in ((23, 19, 17), (64, 64, 61)):
        ai, aj, aa = pkg.poisson_csr(*dims)
        rhs, _ = pkg.poisson_vectors(*dims)
        b = torch.from_numpy(rhs).to(dev)
        out = {}
        for temps in (0, 1):
            with pkg.SeqAIJHIP(ai, aj, aa, row_patterns=temps, row_templates=temps, column_codes=0) as A:
                assert A.info()["row_templates"] == temps
                x = torch.zeros_like(b)
                with K.KSPCG(A, pc="jacobi", rtol=1e-10, max_it=300) as ksp:
                    ksp.set_up()
                    ksp.solve(b, x)
                    torch.cuda.synchronize()
                    out[temps] = (ksp.its, ksp.history(), x.cpu().numpy())
        assert out[0][0] == out[1][0]
        assert_bits(out[0][1], out[1][1])
        assert_bits(out[0][2], out[1][2])


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_golden_patterns(pkg, dev, name):
    """Every golden fixture with patterns requested (taken where they fit):
    rows within the block cap stay bit-identical to the fixture."""
    g = golden(name)
    ai, aj, aa, n = g["ai"], g["aj"], g["aa"], int(g["ncols"])
    with pkg.SeqAIJHIP(ai, aj, aa, ncols=n, row_patterns=1, exact=1) as A:
        xd = to_dev(g["x"], dev)
        y = torch.full((A.m,), np.nan, dtype=torch.float64, device=dev)
        A.mult(xd, y)
        torch.cuda.synchronize()
        short = np.diff(ai) <= A.info()["stream_nnz_cap"]
        assert_bits(y.cpu().numpy(), g["y"], short)


def test_many_patterns_fall_back(pkg, dev, coracle):
    """Short random rows (>256 distinct offset lists): no patterns; the plan
    keeps another layout and the product stays the oracle's."""
    rng = np.random.default_rng(9)
    m = 50000
    lens = rng.integers(3, 9, m)
    cols = [np.unique(np.clip(i + rng.integers(-40, 41, l), 0, m - 1)) for i, l in enumerate(lens)]
    ai = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    aj = np.concatenate(cols).astype(np.int32)
    aa = rng.uniform(-1, 1, len(aj))
    x = rng.uniform(-1, 1, m)
    with pkg.SeqAIJHIP(ai, aj, aa, row_patterns=1) as A:
        assert A.info()["row_patterns"] == 0
        xd = to_dev(x, dev)
        y = torch.empty(m, dtype=torch.float64, device=dev)
        A.mult(xd, y)
        torch.cuda.synchronize()
        assert_bits(y.cpu().numpy(), coracle.matmult(ai, aj, aa, x, omp=True))


def test_many_patterns_plan_time_large(pkg, dev, coracle):
    """a ~10^6-row random short-row operand (far more than 256
    distinct offset lists) must leave the row-pattern attempt early (the
    insert stops once the table has overflowed) instead of probing all 4096
    slots for every row: the plan stays within seconds, the product the
    oracle's."""
    import time
    rng = np.random.default_rng(21)
    m, L = 1_000_000, 6
    offs = -40 + rng.integers(0, 10, (m, 1)) + np.cumsum(rng.integers(1, 14, (m, L)), axis=1)
    cols = np.arange(m)[:, None] + offs
    keep = (cols >= 0) & (cols < m)
    ai = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
    aj = cols[keep].astype(np.int32)
    aa = rng.uniform(-1, 1, len(aj))
    x = rng.uniform(-1, 1, m)
    t0 = time.perf_counter()
    with pkg.SeqAIJHIP(ai, aj, aa, row_patterns=1) as A:
        torch.cuda.synchronize()
        t_plan = time.perf_counter() - t0
        assert A.info()["row_patterns"] == 0
        assert t_plan < 10.0, f"plan took {t_plan:.2f} s"
        xd = to_dev(x, dev)
        y = torch.empty(m, dtype=torch.float64, device=dev)
        A.mult(xd, y)
        torch.cuda.synchronize()
        assert_bits(y.cpu().numpy(), coracle.matmult(ai, aj, aa, x, omp=True))


def test_cg_and_gamg_with_patterns_bitwise(pkg, dev):
    """The solver path on a patterned operator: CG + Jacobi (the fused
    SpMV + p.w epilogue) and CG + GAMG (the fused V-cycle smoothers and the
    set-up's power iteration on the fine level) give the aj run's residual
    history and solution bit for bit, with row patterns and with row
    templates."""
    K = importlib.import_module("petsc-openacc_amd.ksp")
    ai, aj, aa = pkg.poisson_csr(40)
    rhs, _ = pkg.poisson_vectors(40, 40, 40)
    b = torch.from_numpy(rhs).to(dev)
    for pc, kw in (("jacobi", dict(rtol=1e-10, max_it=500)), ("gamg", dict(rtol=1e-14, atol=1e-12))):
        out = {}
        for pats, temps in ((0, 0), (1, 0), (1, 1)):
            with pkg.SeqAIJHIP(ai, aj, aa, row_patterns=pats, row_templates=temps, column_codes=0) as A:
                assert (A.info()["row_patterns"] > 0) == bool(pats)
                assert A.info()["row_templates"] == temps
                x = torch.zeros_like(b)
                with K.KSPCG(A, pc=pc, **kw) as ksp:
                    ksp.set_up()
                    ksp.solve(b, x)
                    torch.cuda.synchronize()
                    assert ksp.fused
                    out[pats, temps] = (ksp.its, ksp.history(), x.cpu().numpy())
        for key in ((1, 0), (1, 1)):
            assert out[0, 0][0] == out[key][0]
            assert_bits(out[0, 0][1], out[key][1])
            assert_bits(out[0, 0][2], out[key][2])


def x_in_row_sized_buffer(x, m, dev):
    """x as the first len(x) entries of a device buffer of max(m, len(x))
    doubles whose tail is NaN: a gather at a row index past the columns (a
    padded template slot) stays inside the buffer, and nothing that is
    summed may come from there."""
    buf = torch.full((max(m, len(x)),), np.nan, dtype=torch.float64, device=dev)
    buf[:len(x)] = to_dev(x, dev)
    return buf[:len(x)]


def assert_products_bitwise(pkg, dev, coracle, ai, aj, aa, n, x, z, expect):
    """MatMult, MatMultAdd and in-place MatMultAdd equal the oracle bit for
    bit on the requested layout and with templates off; `expect` = the
    (row_templates, row_patterns) that info() must report first."""
    m = len(ai) - 1
    y_ref = coracle.matmult(ai, aj, aa, x)
    w_ref = coracle.matmult_add(ai, aj, aa, x, z)
    with pkg.SeqAIJHIP(ai, aj, aa, ncols=n, row_patterns=1) as A:
        info = A.info()
        assert (info["row_templates"], info["row_patterns"]) == expect
        xd, zd = x_in_row_sized_buffer(x, m, dev), to_dev(z, dev)
        for templates in (1, 0):
            if not templates:
                A.set_option("row_templates", 0)
                assert A.info()["row_templates"] == 0
            y = torch.full((m,), np.nan, dtype=torch.float64, device=dev)
            w = torch.full((m,), np.nan, dtype=torch.float64, device=dev)
            wi = zd.clone()
            A.mult(xd, y)
            A.mult_add(xd, zd, w)
            A.mult_add(xd, wi, wi)
            torch.cuda.synchronize()
            assert_bits(y.cpu().numpy(), y_ref)
            assert_bits(w.cpu().numpy(), w_ref)
            assert_bits(wi.cpu().numpy(), w_ref)


RECT_VARIANTS = (((), ()), ((0,), (0.5,)), ((0, 2), (-1.0, 2.0)), ((0, 1, 2), (0.25, -1.0, 0.5)),
                 ((0, 1, 3), (2.0, 0.5, -0.25)))


def tall_rect_csr(m, n, rng):
    """m x n, m >> n: row r takes one of RECT_VARIANTS (none to three
    entries, about 1 in 20 rows none) at column r % (n - 3) + offset, so the
    rows of each run of n - 3 share their column - row offsets and the
    operand has ~ 4 m / (n - 3) + 1 templates."""
    pick = np.where(rng.random(m) < 0.05, 0, rng.integers(1, len(RECT_VARIANTS), m))
    pick[[n + 3, m - 1]] = 0  # empty rows whose index is no column
    cols = [np.array(RECT_VARIANTS[p][0], dtype=np.int64) + r % (n - 3) for r, p in enumerate(pick)]
    vals = [np.array(RECT_VARIANTS[p][1]) for p in pick]
    ai = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    return ai, np.concatenate(cols).astype(np.int32), np.concatenate(vals)


def test_templates_rectangular_with_empty_rows(pkg, dev, coracle):
    """Fewer columns than rows (1537 x 40), some rows empty, some of those
    past the last column: the pipelined launch's padded slots gather the
    template's own first column, and an empty template (which has none)
    sends the operand to the 2-rows-per-lane kernel, whose gathers are per
    entry. x sits in a buffer of m doubles with a NaN tail: every gather
    stays inside it and no product depends on one past x."""
    m, n = 1537, 40
    rng = np.random.default_rng(1537)
    ai, aj, aa = tall_rect_csr(m, n, rng)
    lens = np.diff(ai)
    assert aj.max() < n and lens.max() == 3
    assert 0.03 * m < (lens == 0).sum() < 0.08 * m and (np.flatnonzero(lens == 0) >= n).any()
    rows = np.repeat(np.arange(m), lens)
    temps = {tuple(aj[ai[i]:ai[i + 1]] - rows[ai[i]:ai[i + 1]]) + tuple(aa[ai[i]:ai[i + 1]].view(np.uint64))
             for i in range(m)}
    assert len(temps) <= 256 and len(temps) + sum(len(t) // 2 for t in temps) <= 1024
    x, z = rng.uniform(-1, 1, n), rng.uniform(-1, 1, m)
    assert_products_bitwise(pkg, dev, coracle, ai, aj, aa, n, x, z, (1, len(temps)))


def test_templates_wide_rectangular_one_short_block(pkg, dev, coracle):
    """The transposed shape, 40 x 1537: one row block of fewer than 64 rows,
    every row its own template (none to three entries anywhere in the
    columns), empty rows included — with at least as many columns as rows
    the pipelined launch keeps them (their slots gather x[row])."""
    m, n = 40, 1537
    rng = np.random.default_rng(40)
    palette = np.array([0.5, -1.0, 2.0, 0.25])
    cols = [np.unique(rng.integers(0, n, rng.integers(0, 4))) for _ in range(m)]
    cols[7], cols[39] = cols[7][:0], cols[39][:0]
    vals = [palette[rng.integers(0, 4, len(c))] for c in cols]
    ai = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    aj, aa = np.concatenate(cols).astype(np.int32), np.concatenate(vals)
    lens = np.diff(ai)
    assert lens.max() == 3 and (lens == 0).sum() >= 2
    ntemps = len({tuple(c - r) + tuple(v) for r, (c, v) in enumerate(zip(cols, vals))})
    x, z = rng.uniform(-1, 1, n), rng.uniform(-1, 1, m)
    assert_products_bitwise(pkg, dev, coracle, ai, aj, aa, n, x, z, (1, ntemps))


def capacity_csr(m, ntrip, long_row=None):
    """m x (m + 2): row i holds columns i, i + 1, i + 2 with value triplet
    (7 i + 3) % ntrip of a palette of distinct triplets — one offset list,
    ntrip templates, each of them in every run of ntrip rows. long_row: that
    row gets a fourth entry at i + 3."""
    t = (7 * np.arange(m) + 3) % ntrip
    pal = np.stack([0.5 + np.arange(ntrip) / 256.0, -1.0 - np.arange(ntrip) / 512.0, np.full(ntrip, 0.25)], axis=1)
    cols = [np.arange(i, i + 3) for i in range(m)]
    vals = [pal[k] for k in t]
    if long_row is not None:
        cols[long_row] = np.arange(long_row, long_row + 4)
        vals[long_row] = np.array([3.0, -3.0, 1.5, 0.125])
    ai = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
    return ai, np.concatenate(cols).astype(np.int32), np.concatenate(vals)


@pytest.mark.parametrize("case,ntrip,long_row,templates", [("a", 256, None, 1), ("b", 257, None, 0),
                                                           ("c", 255, 1000, 0)])
def test_template_table_capacity(pkg, dev, coracle, case, ntrip, long_row, templates):
    """The plan's limits, at them and one past: 256 templates (an 8-bit id)
    and 1024 table words (a word and the offsets per template).
    a: 256 templates of 3 entries = 256 + 768 = 1024 words: templates, and
       the last id, 255, on rows of every block (each run of 256 rows holds
       every template), the last block's included;
    b: 257 templates: none; the one offset list stays as a row pattern;
    c: 255 templates of 3 entries and one of 4 = 256 + 769 = 1025 words: none;
       the two offset lists stay as row patterns (info() reports 2).
    MatMult and MatMultAdd bitwise the oracle's in all three."""
    m = 4096
    ai, aj, aa = capacity_csr(m, ntrip, long_row)
    trips = {tuple(aa[ai[i]:ai[i + 1]].view(np.uint64)) for i in range(m)}
    assert len(trips) == ntrip + (long_row is not None)
    assert len({tuple(aa[ai[i]:ai[i + 1]].view(np.uint64)) for i in range(m - 256, m)}) >= min(ntrip, 255)
    words = len(trips) + sum(len(t) for t in trips)
    assert (words <= 1024 and len(trips) <= 256) == bool(templates)
    x, z = pkg.splitmix_uniform(m + 2, 11), pkg.splitmix_uniform(m, 12)
    with pkg.SeqAIJHIP(ai, aj, aa, ncols=m + 2, row_patterns=1) as A:
        info = A.info()
        print(f"case {case}: row_templates {info['row_templates']}, row_patterns {info['row_patterns']}")
        assert info["row_templates"] == templates
        if case == "a":
            assert info["row_patterns"] == 256
        if case == "b":
            assert info["row_patterns"] == 1
        y, w = products(A, x, z, dev)
        assert_bits(y, coracle.matmult(ai, aj, aa, x))
        assert_bits(w, coracle.matmult_add(ai, aj, aa, x, z))


def test_templates_keep_the_sign_of_a_stored_zero(pkg, dev, coracle):
    """Rows that differ only in the sign of a stored 0.0 are two templates
    (the templates hash the value bits): with z = -0.0 and x > 0 MatMultAdd
    gives -0.0 + 0.0 x = +0.0 on the one and -0.0 + (-0.0) x = -0.0 on the
    other, the oracle's bits."""
    m = 700
    ai = np.arange(m + 1, dtype=np.int32)
    aj = np.arange(m, dtype=np.int32)
    aa = np.where(np.arange(m) % 3 == 1, -0.0, 0.0)
    x, z = np.random.default_rng(0).uniform(0.5, 1.0, m), np.full(m, -0.0)
    ref = coracle.matmult_add(ai, aj, aa, x, z)
    assert np.array_equal(np.signbit(ref), np.arange(m) % 3 == 1)
    with pkg.SeqAIJHIP(ai, aj, aa, row_patterns=1) as A:
        info = A.info()
        assert (info["row_templates"], info["row_patterns"]) == (1, 2)
        _, w = products(A, x, z, dev)
        assert_bits(w, ref)
        wi = to_dev(z, dev)
        A.mult_add(to_dev(x, dev), wi, wi)
        torch.cuda.synchronize()
        assert_bits(wi.cpu().numpy(), ref)
