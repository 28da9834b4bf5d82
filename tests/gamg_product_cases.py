"""Operands for the device set-up's sparse products (test_gamg_products.py
checks their shapes on the CPU, test_gamg_products_gpu.py runs them), built
by construction so that each row's distinct output columns are known.

A product row "fits" a hash table of T slots when it never holds more than
keys_max keys: T / 2 for a product of few rows ("half"), T - 1 otherwise
("full"). The rows here come in two makes:
  disjoint  the B rows an A row names share no column, so the distinct
            columns are the sum of their lengths;
  overlap   a few B rows named several times over first (the sum of the
            lengths named passes keys_max, the distinct columns stay below
            half of it), then disjoint B rows up to the count wanted.
"""
from __future__ import annotations

import functools

import numpy as np

TABLES = (16, 32, 64, 128, 256, 1024)
LANES = (4, 8, 16, 32, 64)  # lanes per row <-> B's mean row length in (G / 2, G]
# every (lanes, table) pair the product instantiates
PAIRS = ((4, 16), (8, 16), (4, 32), (8, 32), (16, 32), (4, 64), (4, 128), (4, 256), (8, 64), (8, 128), (8, 256),
         (16, 64), (16, 128), (16, 256), (16, 1024), (32, 64), (32, 128), (32, 256), (32, 1024), (64, 128),
         (64, 256), (64, 1024))
SLAB = 2048  # rows i and i + SLAB fall to the same group of every grid of at most 32 workgroups
HASH_MUL = 0x9E3779B1


REGIMES = ("half", "full")


def same_bits(X, Y):
    """Two CSR triples agree in ai, aj and the bits of aa."""
    return (np.array_equal(X[0], Y[0]) and np.array_equal(X[1], Y[1]) and
            np.array_equal(np.asarray(X[2], np.float64).view(np.uint64), np.asarray(Y[2], np.float64).view(np.uint64)))


def keys_max(T, regime):
    return T // 2 if regime == "half" else T - 1


def table_for(d, regime):
    """The smallest table whose keys_max holds d distinct columns."""
    return next(T for T in TABLES if d <= keys_max(T, regime))


def values(rng, n):
    """+-2^e x a uniform mantissa, e in [-20, 20]: a changed summation order
    or a dropped term changes bits."""
    return rng.choice([-1.0, 1.0], n) * np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(-20, 21, n))


def home_slot(c, T):
    """The product's hash: ((uint32)c * 0x9E3779B1) >> (32 - log2 T)."""
    return ((np.asarray(c, np.uint64) * np.uint64(HASH_MUL)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - T.bit_length() + 1)


def _order(rng, idx, how):
    """Storage order of a row: ascending, reversed or shuffled."""
    idx = np.sort(np.asarray(idx))
    if how % 3 == 1:
        return idx[::-1].copy()
    if how % 3 == 2:
        return rng.permutation(idx)
    return idx


def _csr(rows, rng, vals=True):
    ai = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int32)
    aj = np.concatenate([np.asarray(r, np.int64) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int32)
    return ai, aj, values(rng, len(aj))


class Pool:
    """B rows over disjoint column ranges, by length."""

    def __init__(self):
        self.rows = []     # B's rows: abstract column ids
        self.by_len = {}   # length -> row ids
        self.ncols = 0

    def add(self, length, count=1):
        for _ in range(count):
            self.by_len.setdefault(length, []).append(len(self.rows))
            self.rows.append(np.arange(self.ncols, self.ncols + length))
            self.ncols += length

    def pick(self, d, skip=()):
        """Disjoint rows whose lengths sum to d (the longest first)."""
        out, skip = [], set(skip)
        for L in sorted(self.by_len, reverse=True):
            for r in self.by_len[L]:
                if L <= d and r not in skip and L > 0:
                    out.append(r)
                    d -= L
        assert d == 0, "the pool cannot make this count"
        return out


def _disjoint_row(pool, d):
    return pool.pick(d)


def _overlap_row(pool, d, kmax, rng):
    """d distinct columns, the named lengths passing kmax long before."""
    small = [L for L in sorted(pool.by_len) if 0 < L <= max(1, kmax // 4)]
    base, u = [], 0
    for L in reversed(small):  # a few rows, at most kmax / 2 distinct columns, none longer than kmax / 4
        for r in pool.by_len[L][:2]:
            if u + L <= min(kmax // 2, d - 1):
                base.append(r)
                u += L
    assert base
    reps = -(-(kmax + 1) // u) + 1  # named lengths: reps * u > kmax
    head = list(rng.permutation(np.repeat(base, reps)))
    return head + pool.pick(d - u, skip=base)


@functools.lru_cache(maxsize=None)
def hash_family(G, regime):
    """One operand pair per lanes-per-row bracket and table regime.

    Returns dict(A, B, n, m, k, n_cu, expect={row: table}, d={row: distinct
    columns}, alen={row: entries}, empties=rows that name empty B rows)."""
    rng = np.random.default_rng(1000 * G + (regime == "full"))
    pool = Pool()
    top = 5 * G
    pool.add(top, -(-1023 // top))
    for L in sorted({1, 2, 3, G - 1, G, G + 1} | {1 << j for j in range(1, G.bit_length())}):
        pool.add(L, 4)
    pool.add(1, 8)
    pool.add(0, 2)  # empty B rows
    # windows of 3 G columns whose rows are random subsets: partial overlaps
    nwin, wrows = 4, []
    for w in range(nwin):
        base = pool.ncols
        pool.ncols += 3 * G
        for _ in range(6):
            wrows.append(len(pool.rows))
            pool.rows.append(base + rng.choice(3 * G, size=int(rng.integers(1, G + 2)), replace=False))
    # filler rows bring B's mean row length to 0.58 G, inside (G / 2, G]
    target = 0.58 * G
    while True:
        nz, k = sum(len(r) for r in pool.rows), len(pool.rows) + 1  # (+ the empty last row)
        if nz / k > target + 0.02 * G:
            pool.add(1)
        elif nz / k < target - 0.02 * G:
            pool.add(G)
        else:
            break
    pool.rows.append(np.zeros(0, np.int64))  # B's last row is empty
    k = len(pool.rows)
    # abstract columns -> scattered actual columns
    n = 3 * pool.ncols + 7
    colmap = rng.choice(n, size=pool.ncols, replace=False)
    brows = [_order(rng, colmap[np.asarray(r, np.int64)], q) for q, r in enumerate(pool.rows)]
    B = _csr(brows, rng)

    first, second = [], []  # the special rows of the first slab and their partners SLAB rows on
    expect, dcount = {}, {}

    def add_pair(d):
        kmax_t = keys_max(table_for(d, regime), regime)
        first.append((_disjoint_row(pool, d), d))
        second.append((_overlap_row(pool, d, kmax_t, rng), d))

    prev = 0
    for T in TABLES:
        km = keys_max(T, regime)
        add_pair((prev + 1 + km) // 2 if T > 16 else 3)  # inside the class
        for d in (km - 1, km, km + 1):
            if d <= keys_max(TABLES[-1], regime):
                add_pair(d)
        prev = km
    # A rows of 1, G-1, G, G+1 and 3G+1 entries over the window rows (a B row named twice now and then)
    shapes = []
    for q, length in enumerate((1, G - 1, G, G + 1, 3 * G + 1)):
        shapes.append(list(rng.choice(wrows[(q % nwin) * 6:(q % nwin) * 6 + 6], size=length)))
    rand = [list(rng.choice(wrows[(q % nwin) * 6:(q % nwin) * 6 + 6], size=int(rng.integers(1, 4)))) for q in range(12)]

    m = 2 * SLAB
    arows = [np.zeros(0, np.int64) for _ in range(m)]
    alen = {}
    for slab, specials in ((0, first), (1, second)):
        for q, (named, d) in enumerate(specials):
            i = slab * SLAB + 3 * q + 1  # empty rows between the full ones
            arows[i] = np.asarray(named, np.int64)
            expect[i] = table_for(d, regime)
            dcount[i] = d
    # A rows that name B's empty rows (z0, z1 and B's last row), in the order written here: first, in the
    # middle and last in a row, in a chunk of fewer than G entries, in a full chunk, and alone
    z0, z1 = pool.by_len[0]
    last = k - 1
    w = [int(r) for r in rng.choice(wrows[:6], size=G)]  # one window: at most 3 G distinct columns
    empties = [[z0, w[0], last],
               [last],
               [w[1], z1, w[2]],
               [last, pool.by_len[G][0], z0, pool.by_len[G + 1][0], pool.by_len[1][0], z1],
               [z1] + w[:G // 2] + [last] + w[G // 2:] + [z0]]  # G + 3 entries: a full chunk, then 3
    at = 3 * len(first) + 5
    fixed = set()  # rows kept in the order they were built in
    for q, named in enumerate(shapes + rand + empties):
        i = (q % 2) * SLAB + at + 2 * q
        arows[i] = np.asarray(named, np.int64)
        if q < len(shapes):
            alen[i] = len(named)
        if q >= len(shapes) + len(rand):
            fixed.add(i)
    # storage order of A's rows: as built (the overlap rows are shuffled), sorted by k, or reversed
    for i in range(m):
        if len(arows[i]) and not (i in expect and i >= SLAB) and i not in fixed:
            arows[i] = _order(rng, arows[i], i)
    A = _csr(arows, rng)
    return dict(A=A, B=B, n=n, m=m, k=k, G=G, regime=regime, n_cu=0 if regime == "half" else 1, expect=expect,
                d=dcount, alen=alen, empties=sorted(fixed))


@functools.lru_cache(maxsize=None)
def probing_case(regime):
    """Rows whose columns all share one home slot in every table: the last
    slot (the chain wraps to slot 0) or one in the middle, with columns up to
    INT32_MAX - 1. B rows of 5..8 entries; row r of `expect` fills table
    expect[r] to its keys_max."""
    rng = np.random.default_rng(77 + (regime == "full"))
    n = 2**31 - 1
    inv = pow(HASH_MUL, -1, 2**32)

    def colliding(top10, count):
        # columns c < 2^31 with ((uint32)c * HASH_MUL) >> 22 == top10: the same home slot in every table
        v = (np.uint64(top10) << np.uint64(22)) + np.arange(1 << 22, dtype=np.uint64)
        c = (v * np.uint64(inv)) & np.uint64(0xFFFFFFFF)
        c = np.sort(c[c < np.uint64(n)]).astype(np.int64)
        return np.concatenate((c[:count - 8], c[-8:]))  # the largest (near INT32_MAX) among them

    last, mid = colliding(0x3FF, 1023), colliding(0x155, 1023)
    brows, sets = [], {}
    for name, cols in (("last", last), ("mid", mid)):
        cols = rng.permutation(cols)
        ids, at = [], 0
        while at < len(cols):
            L = int(rng.integers(5, 9)) if len(cols) - at > 40 else 1  # singles at the end: any count can be made
            ids.append(len(brows))
            brows.append(_order(rng, cols[at:at + L], len(brows)))
            at += L
        sets[name] = ids
    brows.append(np.asarray([n - 1]))  # the largest column index there is
    big = len(brows) - 1
    lens = np.array([len(r) for r in brows])

    def take(ids, d):
        out = []
        for r in ids:
            if lens[r] <= d:
                out.append(r)
                d -= lens[r]
        assert d == 0
        return out

    m = 512
    arows = [np.zeros(0, np.int64) for _ in range(m)]
    expect, slot = {}, {}
    i = 1
    for T in TABLES:
        km = keys_max(T, regime)
        for name in ("last", "mid"):
            arows[i] = np.asarray(take(sets[name], km))
            expect[i], slot[i] = T, name
            i += 5
        # both chains in one table, and the largest column
        arows[i] = np.asarray(take(sets["last"], km // 2) + take(sets["mid"], km - km // 2 - 1) + [big])
        expect[i], slot[i] = T, "both"
        i += 5
    B = _csr(brows, rng)
    A = _csr(arows, rng)
    return dict(A=A, B=B, n=n, m=m, k=len(brows), regime=regime, n_cu=0 if regime == "half" else 1, expect=expect,
                slot=slot, last=last, mid=mid)


@functools.lru_cache(maxsize=None)
def too_wide_case(regime):
    """One row with a distinct column more than the largest table holds
    (1025 with full tables, 513 with half-full ones) among ordinary rows."""
    rng = np.random.default_rng(5)
    d = 1025 if regime == "full" else 513
    brows = [np.arange(8 * r, 8 * r + 8) for r in range(130)] + [np.asarray([1040])]
    m = 256
    arows = [rng.choice(130, size=2) for _ in range(m)]
    arows[100] = np.concatenate((np.arange(d // 8), [130]))
    return dict(A=_csr(arows, rng), B=_csr(brows, rng), n=1041, m=m, k=len(brows), d=d, row=100,
                n_cu=0 if regime == "half" else 1)


@functools.lru_cache(maxsize=None)
def p0_case(name):
    """A (m x k), agg[k], p0[k]: "fits" every row has at most 8 distinct
    aggregates among its columns (rows with 0, 1, 7 and 8 present) and A at
    most 8 entries per row; "nine": the same with one row of 9; "dense": A
    has more than 8 entries per row."""
    rng = np.random.default_rng({"fits": 11, "nine": 12, "dense": 13}[name])
    m, k, na = 600, 700, 90
    agg = rng.integers(0, na, k).astype(np.int32)
    agg[rng.choice(k, 60, replace=False)] = -1  # rows no aggregate took
    agg[:6] = -1
    by_agg = [np.flatnonzero(agg == a) for a in range(na)]

    def row(ndistinct, per):
        """`per` columns from each of ndistinct aggregates, interleaved."""
        aggs = rng.choice(na, ndistinct, replace=False)
        cols = np.concatenate([rng.choice(by_agg[a], per) for a in aggs] + [np.zeros(0, np.int64)])
        return rng.permutation(cols)

    arows = []
    if name == "dense":
        for i in range(m):
            arows.append(np.concatenate((row(int(rng.integers(1, 8)), 3), rng.choice(6, 2))))
    else:
        for i in range(m):
            nd = int(rng.integers(0, 5))
            arows.append(np.concatenate((row(nd, 1), rng.choice(6, int(rng.integers(0, 2))))))
        arows[3] = np.asarray([0, 1, 2])          # columns without an aggregate only: 0 distinct
        arows[4] = np.zeros(0, np.int64)          # an empty row
        arows[5] = row(1, 6)                      # one aggregate, six terms
        arows[300] = row(7, 1)
        arows[301] = np.concatenate((row(8, 1)[:8], [4]))   # 8 distinct (8 entries + one without an aggregate = 9 > 8)
        arows[302] = row(4, 2)                    # sums accumulate
        arows[599] = row(8, 1)
        if name == "nine":
            arows[303] = row(9, 1)
    arows = [_order(rng, r, i) if i % 4 else np.asarray(r, np.int64) for i, r in enumerate(arows)]
    A = _csr(arows, rng)
    distinct = np.array([len(set(agg[r][agg[r] >= 0].tolist())) for r in arows])
    return dict(A=A, agg=agg, p0=values(rng, k), na=na, m=m, k=k, distinct=distinct)


@functools.lru_cache(maxsize=None)
def prolong_case():
    """T (m x n, ascending columns, some past the na local aggregates), agg,
    p0, dinv, alpha < 0, and `where`[i]: agg[i] relative to T's row i."""
    rng = np.random.default_rng(21)
    m, na, n = 400, 60, 75  # columns [na, n): ghost coarse columns
    trows, agg, where = [], np.empty(m, np.int32), []
    kinds = ("below", "between", "on", "above", "none", "empty+agg", "empty-agg", "ghost")
    for i in range(m):
        kind = kinds[i % len(kinds)]
        if kind.startswith("empty"):
            cols = np.zeros(0, np.int64)
            agg[i] = rng.integers(0, na) if kind == "empty+agg" else -1
        else:
            hi = n if kind == "ghost" else na
            cols = np.sort(rng.choice(np.arange(5, hi - 5), size=int(rng.integers(2, 9)), replace=False))
            if kind == "ghost":
                cols[-1] = n - 1
            if kind == "below":
                agg[i] = rng.integers(0, cols[0])
            elif kind == "above":
                agg[i] = rng.integers(cols[-1] + 1, na)
            elif kind == "ghost":
                agg[i] = rng.integers(0, na)
            elif kind == "on":
                agg[i] = rng.choice(cols)
            elif kind == "none":
                agg[i] = -1
            else:  # a gap between two of T's columns
                gaps = [c for c in range(cols[0] + 1, cols[-1]) if c not in cols]
                agg[i] = gaps[0] if gaps else cols[0]
        trows.append(cols)
        where.append(kind)
    T = _csr(trows, rng)
    return dict(T=T, n=n, na=na, m=m, agg=agg, p0=values(rng, m), dinv=values(rng, m), alpha=-0.7368421052631579,
                where=where)


@functools.lru_cache(maxsize=None)
def tentative_case():
    """Aggregates of 1, 2, 63, 64, 65 and 1000 members spread through the
    rows, one without members, one whose B is all 0, many small ones (more
    than one block of aggregates), and rows no aggregate took."""
    rng = np.random.default_rng(31)
    sizes = [1, 2, 63, 64, 65, 1000, 0, 7] + [int(s) for s in rng.integers(1, 4, 300)]
    na = len(sizes)
    agg = np.concatenate([np.full(s, a) for a, s in enumerate(sizes)] + [np.full(40, -1)]).astype(np.int32)
    agg = rng.permutation(agg)
    B = values(rng, len(agg))
    B[agg == 7] = 0.0
    return dict(agg=agg, B=B, na=na, sizes=np.asarray(sizes), zero=7, empty=6)
