"""MatMatMult (aijhip_mat_mat_mult): Y = A X for a block of k dense vectors,
the matrix read once per chunk of up to 8 columns. Every Y(i, j) is the PETSc
row loop's value on column j (s = 0.0, then s += aa[p] * X(aj[p], j) in
storage order), so every result must be BIT-IDENTICAL to the oracle
(oracle/matmult_seqaij.c) on that column: for each of the three paths (row
templates, CSR row blocks, generic rows), both dense layouts, every chunk
width, tight and padded leading dimensions, and X 16-byte aligned or not.
Each test asserts the path its operand takes, so that a fallback cannot hide
a broken fast kernel."""

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = -7.25
KS_A = (1, 2, 3, 4, 7, 8, 9)
# sweep A: every k, both layouts, tight and padded leading dimensions, X aligned and 8 bytes in
SWEEP_A = [(k, lay, pad, mis) for k in KS_A for lay in ("interleaved", "columns") for pad in (False, True)
           for mis in (False, True)]
# sweep B: one layout per k
SWEEP_B = [(2, "interleaved", True, False), (3, "columns", True, True), (8, "interleaved", False, True),
           (8, "columns", False, False)]
NO_TEMPLATES = dict(row_templates=0, row_patterns=0, column_codes=0)


@pytest.fixture(scope="module")
def dev(pkg):
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch.device("cuda:0")


def assert_bits(a, b):
    a, b = np.ascontiguousarray(a).ravel(), np.ascontiguousarray(b).ravel()
    assert a.shape == b.shape
    bad = np.nonzero(a.view(np.uint64) != b.view(np.uint64))[0]
    assert bad.size == 0, f"{bad.size}/{a.size} entries differ bitwise; first {bad[:4]}: {a[bad[:4]]} vs {b[bad[:4]]}"


class Operand:
    """A host CSR with its oracle products, computed once per k and shared."""

    def __init__(self, pkg, coracle, ai, aj, aa, ncols=None, seed=42):
        self.pkg, self.coracle = pkg, coracle
        self.ai, self.aj, self.aa = ai, aj, np.asarray(aa, dtype=np.float64)
        self.m = len(ai) - 1
        self.n = self.m if ncols is None else ncols
        self.seed = seed
        self._ref = {}

    def with_values(self, aa):
        return Operand(self.pkg, self.coracle, self.ai, self.aj, aa, self.n, self.seed)

    def x(self, k):
        return self.pkg.splitmix_uniform(self.n * k, self.seed + k).reshape(self.n, k)

    def ref(self, k):
        if k not in self._ref:
            X = self.x(k)
            Y = np.stack([self.coracle.matmult(self.ai, self.aj, self.aa, X[:, j]) for j in range(k)], axis=1)
            Y.setflags(write=False)
            self._ref[k] = Y
        return self._ref[k]


def dense_block(rows, k, layout, pad, offset, dev, fill):
    """(buffer, view, ld): a rows x k block of the layout inside a flat buffer
    filled with `fill`, its leading dimension padded (interleaved k + 1,
    columns rows + 3) or tight, starting `offset` elements into the buffer."""
    ld = (k + 1 if pad else k) if layout == "interleaved" else (rows + 3 if pad else rows)
    count = rows * ld if layout == "interleaved" else k * ld
    buf = torch.full((count + offset + 1,), fill, dtype=torch.float64, device=dev)
    assert buf.data_ptr() % 16 == 0
    flat = buf[offset:offset + count]
    view = flat.view(rows, ld)[:, :k] if layout == "interleaved" else flat.view(k, ld).t()[:rows, :]
    assert view.shape == (rows, k) and view.data_ptr() == buf.data_ptr() + 8 * offset
    return buf, view, ld


def run_case(A, op, k, layout, pad, misaligned, dev):
    """One mat_mult: the m x k block equals the oracle bit for bit and nothing else of Y's buffer is written."""
    _, X, _ = dense_block(op.n, k, layout, pad, 1 if misaligned else 0, dev, np.nan)
    X.copy_(torch.from_numpy(op.x(k)).to(dev))
    ybuf, Y, ld = dense_block(op.m, k, layout, pad, 0, dev, SENTINEL)
    A.mat_mult(X, Y)
    torch.cuda.synchronize()
    yh = ybuf.cpu().numpy()
    i, j = np.meshgrid(np.arange(op.m), np.arange(k), indexing="ij")
    inside = (i * ld + j if layout == "interleaved" else i + j * ld).ravel()
    assert_bits(yh[inside], op.ref(k))
    outside = np.ones(yh.size, dtype=bool)
    outside[inside] = False
    assert outside.sum() == yh.size - op.m * k
    assert np.all(yh[outside] == SENTINEL), "mat_mult wrote outside the m x k block"


def sweep(A, op, cases, dev, path):
    for k in sorted({c[0] for c in cases}):
        for lay in ("interleaved", "columns"):
            plan = A.mat_mult_plan(k, lay)
            assert plan["path"] == path, (plan, A.info())
            assert plan["n_chunks"] == len(op.pkg.chunk_widths(k))
    for k, lay, pad, mis in cases:
        try:
            run_case(A, op, k, lay, pad, mis, dev)
        except AssertionError as e:
            raise AssertionError(f"k={k} layout={lay} padded={pad} misaligned={mis}: {e}") from e


def box_stencil_csr(nz, ny, nx):
    """Constant-coefficient box stencil (9 points with nz = 1) on an
    nz x ny x nx grid: the point count less one on the diagonal, -1 off it."""
    idx = np.arange(nz * ny * nx).reshape(nz, ny, nx)
    rows, cols, vals = [], [], []
    dzs = (-1, 0, 1) if nz > 1 else (0,)
    npts = 9 * len(dzs)

    def sl(d, n):
        return slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d))

    for dz in dzs:
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
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


def prolongator_csr(m=250, n=17):
    """m x n, n < m, one to three entries a row with values of their own: every row is its own template."""
    rng = np.random.default_rng(m)
    rows = [np.unique(rng.integers(0, n, rng.integers(1, 4))) for _ in range(m)]
    vals = [rng.uniform(-1, 1, len(c)) for c in rows]
    ai = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int32)
    return ai, np.concatenate(rows).astype(np.int32), np.concatenate(vals)


def cap_edge_csr(last_row_nnz, ncols=5000):
    """64 rows of 1023 entries, then one row of last_row_nnz entries, over ncols columns."""
    rng = np.random.default_rng(last_row_nnz)
    lens = [1023] * 64 + [last_row_nnz]
    ai = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    aj = rng.integers(0, ncols, ai[-1]).astype(np.int32)
    return ai, aj, rng.uniform(-1, 1, ai[-1])


POISSON_DIMS = [(20, 17, 13), (1, 9, 40), (300, 2, 3)]


@pytest.fixture(scope="module")
def poisson_ops(pkg, coracle):
    return {d: Operand(pkg, coracle, *pkg.poisson_csr(*d)) for d in POISSON_DIMS}


@pytest.fixture(scope="module")
def fem_op(pkg, coracle):
    return Operand(pkg, coracle, *pkg.fem_hex_csr(5, 4, 3, dofs=3))


@pytest.fixture(scope="module")
def golden_ops(pkg, coracle):
    out = {}
    for name in ("skewed_small", "compressed_small"):
        g = golden(name)
        out[name] = Operand(pkg, coracle, g["ai"], g["aj"], g["aa"], int(g["ncols"]))
    return out


def make(pkg, op, **options):
    return pkg.SeqAIJHIP(op.ai, op.aj, op.aa, ncols=op.n, **options)


# ---- path 2: row templates
@pytest.mark.parametrize("dims", POISSON_DIMS)
def test_templates_poisson(pkg, dev, poisson_ops, dims):
    """1: 7-point Poisson on a box and two thin grids; the last row block is partial."""
    op = poisson_ops[dims]
    with make(pkg, op) as A:
        assert A.info()["row_templates"] == 1
        sweep(A, op, SWEEP_A, dev, path=2)


def test_templates_nine_entry_rows(pkg, dev, coracle):
    """2: the 2-D 9-point box stencil: templates past the pipelined MatMult kernel's 8 slots."""
    op = Operand(pkg, coracle, *box_stencil_csr(1, 40, 37))
    assert np.diff(op.ai).max() == 9
    with make(pkg, op) as A:
        assert A.info()["row_templates"] == 1
        sweep(A, op, SWEEP_A, dev, path=2)


def test_templates_rectangular(pkg, dev, coracle):
    """3: 250 x 17, every row its own template; X has only 17 rows."""
    op = Operand(pkg, coracle, *prolongator_csr(250, 17), ncols=17)
    with make(pkg, op, row_patterns=1) as A:
        assert A.info()["row_templates"] == 1
        sweep(A, op, SWEEP_A, dev, path=2)


# ---- path 1: CSR row blocks
@pytest.mark.parametrize("dims", POISSON_DIMS)
def test_csr_poisson(pkg, dev, poisson_ops, dims):
    """4: the same operands from aj / aa, then with random values."""
    op = poisson_ops[dims]
    with make(pkg, op, **NO_TEMPLATES) as A:
        inf = A.info()
        assert (inf["row_templates"], inf["row_patterns"], inf["column_codes"]) == (0, 0, 0)
        sweep(A, op, SWEEP_A, dev, path=1)
        op2 = op.with_values(np.random.default_rng(5).uniform(-1, 1, len(op.aa)))
        A.update_values(op2.aa)
        sweep(A, op2, SWEEP_A, dev, path=1)


def test_csr_fem_rows(pkg, dev, fem_op):
    """5: 81-entry rows, blocks of few rows, whatever layout MatMult itself reads."""
    assert np.diff(fem_op.ai).max() == 81
    with make(pkg, fem_op) as A:
        sweep(A, fem_op, SWEEP_A, dev, path=1)


def test_csr_cap_edge(pkg, dev, coracle):
    """6: a row of exactly the geometry's 4094-entry cap is a block of its own, summed by one lane in order."""
    op = Operand(pkg, coracle, *cap_edge_csr(4094), ncols=5000)
    with make(pkg, op, geometry=6) as A:
        assert A.info()["n_long_rows"] == 0
        sweep(A, op, SWEEP_A, dev, path=1)


# ---- path 0: generic rows
def test_generic_past_the_cap(pkg, dev, coracle):
    """7: one entry more and the row leaves the row blocks: generic rows."""
    op = Operand(pkg, coracle, *cap_edge_csr(4095), ncols=5000)
    with make(pkg, op, geometry=6) as A:
        assert A.info()["n_long_rows"] >= 1
        sweep(A, op, SWEEP_B, dev, path=0)


@pytest.mark.parametrize("name", ["skewed_small", "compressed_small"])
def test_generic_goldens(pkg, dev, golden_ops, name):
    """8: the skewed golden's longest rows (up to 2500 entries) are long rows
    at geometry 0's 2048-entry cap; compressed rows, whose empty rows give
    +0.0. The skewed golden once more on its automatic plan, whose path follows
    from whether it has long rows."""
    op = golden_ops[name]
    with make(pkg, op, **({"geometry": 0} if name == "skewed_small" else {})) as A:
        inf = A.info()
        assert inf["n_long_rows"] >= 1 if name == "skewed_small" else inf["compressed_row"] == 1
        sweep(A, op, SWEEP_B, dev, path=0)
    if name == "skewed_small":
        with make(pkg, op) as A:
            sweep(A, op, SWEEP_B, dev, path=0 if A.info()["n_long_rows"] else 1)
    if name == "compressed_small":
        empty = np.diff(op.ai) == 0
        assert empty.any()
        assert not np.signbit(op.ref(2)[empty]).any()  # +0.0 is what the sweep compared against


def test_generic_scalar_plan(pkg, dev, fem_op):
    """9: a SCALAR plan has no row blocks."""
    with make(pkg, fem_op) as A:
        A.set_kernel("scalar")
        sweep(A, fem_op, SWEEP_B, dev, path=0)


def test_generic_wide_geometry(pkg, dev, fem_op):
    """10: geometry 7's blocks hold up to 8190 entries, more than the CSR path stages."""
    with make(pkg, fem_op) as A:
        A.set_option("geometry", 7)
        sweep(A, fem_op, SWEEP_B, dev, path=0)


# ---- the plan's figures
def test_plan_bytes(pkg, dev, poisson_ops, golden_ops):
    """bytes = sum over the chunks of M, plus 8 k (n + m): M from mult_bytes
    (paths 0 and 1) or mult_layout_bytes (path 2), each less its vectors."""
    p = poisson_ops[(20, 17, 13)]
    for op, options, path, key in ((p, {}, 2, "mult_layout_bytes"), (p, NO_TEMPLATES, 1, "mult_bytes"),
                                   (golden_ops["skewed_small"], {"geometry": 0}, 0, "mult_bytes")):
        with make(pkg, op, **options) as A:
            inf = A.info()
            M = inf[key] - 8 * op.n - 8 * op.m
            if path != 2:
                assert M == 12 * len(op.aj) + 4 * (op.m + 1)
            for k in (0, 1, 7, 8, 19):
                for lay in ("interleaved", "columns"):
                    plan = A.mat_mult_plan(k, lay)
                    assert plan["path"] == path
                    assert plan["n_chunks"] == len(pkg.chunk_widths(k))
                    assert plan["bytes"] == plan["n_chunks"] * M + 8 * k * (op.n + op.m)


@pytest.mark.parametrize("options", [{}, NO_TEMPLATES], ids=["templates", "csr"])
def test_columns_equal_mult(pkg, dev, poisson_ops, options):
    """Every column of mat_mult is mult of that column, bit for bit (operands 1 and 4)."""
    op = poisson_ops[(20, 17, 13)]
    k = 9
    Xh = op.x(k)
    with make(pkg, op, **options) as A:
        X = torch.from_numpy(Xh).to(dev)
        Y = torch.full((op.m, k), np.nan, dtype=torch.float64, device=dev)
        A.mat_mult(X, Y)
        y = torch.full((op.m,), np.nan, dtype=torch.float64, device=dev)
        for j in range(k):
            A.mult(X[:, j].contiguous(), y)
            torch.cuda.synchronize()
            assert_bits(Y[:, j].cpu().numpy(), y.cpu().numpy())


@pytest.mark.parametrize("order", ["C", "F"])
def test_host_form(pkg, dev, poisson_ops, golden_ops, order):
    """mat_mult_host with C-order (interleaved) and F-order (columns) numpy arrays equals the oracle."""
    for op, options in ((poisson_ops[(20, 17, 13)], {}), (golden_ops["skewed_small"], {"geometry": 0})):
        with make(pkg, op, **options) as A:
            for k in (3, 8):
                X = np.array(op.x(k), order=order)
                Y = A.mat_mult_host(X)
                assert Y.shape == (op.m, k) and Y.flags[f"{order}_CONTIGUOUS"]
                assert_bits(Y, op.ref(k))
                out = np.full((op.m, k + 2), SENTINEL, order=order)
                assert A.mat_mult_host(X, out=out[:, :k]) is not None
                assert_bits(out[:, :k], op.ref(k))
                assert np.all(out[:, k:] == SENTINEL)


def test_errors_on_a_live_handle(pkg, dev, poisson_ops):
    op = poisson_ops[(1, 9, 40)]
    L = pkg.lib()
    k = 4
    with make(pkg, op) as A:
        X = torch.from_numpy(op.x(k)).to(dev)
        Y = torch.full((op.m, k), SENTINEL, dtype=torch.float64, device=dev)
        s = torch.cuda.current_stream().cuda_stream

        def call(kk, layout, x, ldx, y, ldy):
            return L.aijhip_mat_mat_mult(A._h, kk, layout, x.data_ptr(), ldx, y.data_ptr(), ldy, s)

        for args in ((k, 1, X, k - 1, Y, k), (k, 1, X, k, Y, k - 1), (k, 0, X, op.n - 1, Y, op.m),
                     (k, 0, X, op.n, Y, op.m - 1), (-1, 1, X, k, Y, k), (k, 2, X, k, Y, k), (k, 1, X, k, X, k)):
            assert call(*args) == pkg.AIJHIP_ERR_ARG, args
            assert L.aijhip_last_error()
        with pytest.raises(pkg.AIJHIPError) as ei:
            A.mat_mult(X, X)
        assert ei.value.code == pkg.AIJHIP_ERR_ARG
        with pytest.raises(pkg.AIJHIPError) as ei:
            pkg._check(call(-1, 1, X, k, Y, k))
        assert ei.value.code == pkg.AIJHIP_ERR_ARG
        with pytest.raises(pkg.AIJHIPError) as ei:
            pkg._check(call(k, 1, X, k - 1, Y, k))
        assert ei.value.code == pkg.AIJHIP_ERR_ARG
        with pytest.raises(pkg.AIJHIPError):
            pkg._check(L.aijhip_mat_mat_mult(A._h, k, 1, None, k, Y.data_ptr(), k, s))
        with pytest.raises(TypeError):  # one layout for both
            A.mat_mult(X, torch.empty((k, op.m), dtype=torch.float64, device=dev).t())
        # k = 0 launches nothing
        assert call(0, 1, X, k, Y, k) == pkg.AIJHIP_OK
        A.mat_mult(X[:, :0], Y[:, :0])
        torch.cuda.synchronize()
        assert bool((Y == SENTINEL).all())
