"""The reference the device products are compared with (oracle/gamg.py
rowprod_ref and friends) agrees with scipy's csr product and with the host
builder, and the operands of gamg_product_cases.py have the shapes their
names promise. CPU only; test_gamg_products_gpu.py runs them on the device."""
import importlib

import numpy as np
import pytest
import scipy.sparse as sp

import gamg_product_cases as cases
from gamg_product_cases import REGIMES, same_bits
from oracle import gamg as ogamg


def product_operands():
    """(id, A, B) of every product the GPU module runs."""
    for G in cases.LANES:
        for regime in REGIMES:
            c = cases.hash_family(G, regime)
            yield f"family-{G}-{regime}", c["A"], c["B"]
    for regime in REGIMES:
        c = cases.probing_case(regime)
        yield f"probing-{regime}", c["A"], c["B"]
        c = cases.too_wide_case(regime)
        yield f"too-wide-{regime}", c["A"], c["B"]
    for name in ("fits", "nine", "dense"):
        c = cases.p0_case(name)
        yield f"p0-{name}", c["A"], ogamg.p0_csr_ref(c["agg"], c["p0"])


def scipy_product(A, B):
    """scipy's csr_matmat with sorted rows. Its accumulators are dense over
    B's columns, so the columns in use are renumbered by rank first (the
    product depends on their order alone) and mapped back."""
    ai, aj, aa = A
    bi, bj, ba = B
    used, rank = np.unique(bj, return_inverse=True)
    C = sp.csr_matrix((aa, aj, ai), shape=(len(ai) - 1, len(bi) - 1)) @ \
        sp.csr_matrix((ba, rank.astype(np.int32), bi), shape=(len(bi) - 1, max(len(used), 1)))
    C.sort_indices()
    return C.indptr, used[C.indices] if len(used) else C.indices, C.data


def distinct_per_row(A, B):
    """Distinct output columns of each row of A B (numpy sets)."""
    ai, aj, _ = A
    bi, bj, _ = B
    return np.array([len(np.unique(np.concatenate([bj[bi[k]:bi[k + 1]] for k in aj[ai[i]:ai[i + 1]]] +
                                                  [np.zeros(0, np.int32)]))) for i in range(len(ai) - 1)])


@pytest.mark.parametrize("name", [o[0] for o in product_operands()])
def test_reference_product_equals_scipy_bitwise(name):
    A, B = next(o[1:] for o in product_operands() if o[0] == name)
    assert same_bits(ogamg.rowprod_ref(A, B), scipy_product(A, B))


def test_reference_product_keeps_cancelled_columns_and_empty_rows():
    A = (np.array([0, 2, 2, 3], np.int32), np.array([0, 1, 1], np.int32), np.array([1.0, -1.0, 2.0]))
    B = (np.array([0, 1, 3], np.int32), np.array([4, 4, 2], np.int32), np.array([3.0, 3.0, 5.0]))
    ci, cj, ca = ogamg.rowprod_ref(A, B)
    assert ci.tolist() == [0, 2, 2, 4] and cj.tolist() == [2, 4, 2, 4]
    assert ca.tolist() == [-5.0, 0.0, 10.0, 6.0]  # column 4 of row 0 sums to 0.0 and stays


@pytest.mark.parametrize("dims", [(8, 8, 8), (6, 7, 5)])
def test_reference_equals_the_host_builder(pkg, dims):
    """The Galerkin operator of every build_host level, recomputed from its A
    and P by the reference (P^T: the stable transpose), bit for bit; and the
    prolongator from the reference's own A P0 and tentative parts."""
    G = importlib.import_module("petsc-openacc_amd.gamg")
    ai, aj, aa = pkg.poisson_csr(*dims)
    lv = G.build_host(ai, aj, aa, coarse_eq_limit=20)
    assert len(lv) >= 2
    A = (ai, aj, aa)
    B = np.ones(len(ai) - 1)
    for l in range(len(lv) - 1):
        m, mc = lv[l]["m"], lv[l + 1]["m"]
        P = lv[l]["P"]
        PT = sp.csr_matrix((P[2], P[1], P[0]), shape=(m, mc)).T.tocsr()
        PT.sort_indices()
        Ac = ogamg.rowprod_ref((PT.indptr, PT.indices, PT.data), ogamg.rowprod_ref(A, P))
        assert same_bits(Ac, lv[l + 1]["A"])
        # the prolongator itself, from its parts
        agg = lv[l]["agg"]
        Bc, p0, _ = ogamg.tentative_ref(agg, B, mc)
        d = ogamg.first_diagonal(sp.csr_matrix((A[2], A[1], A[0]), shape=(m, m)))
        dinv = 1.0 / np.where(d == 0.0, 1.0, d)
        T = ogamg.rowprod_ref(A, ogamg.p0_csr_ref(agg, p0))
        assert same_bits(ogamg.prolong_ref(T, agg, p0, dinv, -1.4 / lv[l]["emax"]), P)
        A, B = lv[l + 1]["A"], Bc


# ---- the shapes the case names promise (numpy only; the product's own
# selection rule is not restated: the GPU tests read what ran from its report)

@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("G", cases.LANES)
def test_family_shape(G, regime):
    c = cases.hash_family(G, regime)
    (ai, aj, aa), (bi, bj, ba) = c["A"], c["B"]
    m, k = len(ai) - 1, len(bi) - 1
    assert (m, k) == (c["m"], c["k"]) and k != m and c["n"] != m and m >= 64 and m <= 4096
    assert bj.max() < c["n"] and aj.max() < k
    blen = np.diff(bi)
    assert G / 2 < blen.mean() <= G  # the bracket this family is for
    assert {0, 1, G, G + 1, 5 * G} <= set(blen.tolist()) and blen[-1] == 0
    # ... and A names rows of those lengths, the empty last row among them: the product sees B through A alone
    assert {0, 1, G, G + 1, 5 * G} <= set(blen[aj].tolist()) and k - 1 in aj
    where = set()  # an empty B row first, in the middle, last and alone in an A row; in a short and in a full chunk
    for i in c["empties"]:
        named = aj[ai[i]:ai[i + 1]]
        for pos in np.flatnonzero(blen[named] == 0):
            where.add("alone" if len(named) == 1 else "first" if pos == 0 else "last" if pos == len(named) - 1
                      else "middle")
            chunk = min(G, len(named) - pos // G * G)  # entries of the G-entry chunk this one lies in
            where.add("short chunk" if chunk < G else "full chunk")
            where.add("last row" if named[pos] == k - 1 else "inner row")
    assert where == {"alone", "first", "middle", "last", "short chunk", "full chunk", "last row", "inner row"}
    for r in range(k):  # a B row holds a column once
        assert len(np.unique(bj[bi[r]:bi[r + 1]])) == blen[r]
    # most rows are short: the mean products per row stay below what the smallest table holds
    products = blen[aj].sum()
    assert products <= 1e5
    assert len(aj) * blen.mean() / m < cases.keys_max(16, regime)
    assert np.count_nonzero(np.diff(ai) == 0) > m // 2  # empty rows between the others
    d = distinct_per_row(c["A"], c["B"])
    assert d.max() == cases.keys_max(cases.TABLES[-1], regime)  # no row past the largest table
    for i, want in c["d"].items():
        assert d[i] == want
    alen = np.diff(ai)
    assert sorted(alen[i] for i in c["alen"]) == [1, G - 1, G, G + 1, 3 * G + 1]
    # every table's class: rows inside it and at keys_max - 1, keys_max, keys_max + 1, each made both ways
    prev = 0
    for T in cases.TABLES:
        km = cases.keys_max(T, regime)
        for slab in (0, 1):
            have = sorted(c["d"][i] for i in c["expect"] if c["expect"][i] == T and i // cases.SLAB == slab)
            assert {km - 1, km} <= set(have) and any(prev + 1 < x < km - 1 for x in have)
            if T != cases.TABLES[-1]:
                assert km + 1 in [c["d"][i] for i in c["expect"] if i // cases.SLAB == slab]
            assert all(prev < x <= km for x in have)
        prev = km
    # the overlap make: the lengths named pass keys_max although the distinct columns fit, and every B
    # row's own length fits beside the columns already there
    for i, T in c["expect"].items():
        if i < cases.SLAB:
            assert blen[aj[ai[i]:ai[i + 1]]].sum() == c["d"][i]  # disjoint B rows
            continue
        km = cases.keys_max(T, regime)
        seen = set()
        for kk in aj[ai[i]:ai[i + 1]]:
            assert len(seen) + blen[kk] <= km
            seen |= set(bj[bi[kk]:bi[kk + 1]].tolist())
        assert blen[aj[ai[i]:ai[i + 1]]].sum() > km >= len(seen)
        assert len(set(aj[ai[i]:ai[i + 1]].tolist())) < alen[i]  # a B row named more than once
        assert i - cases.SLAB in c["expect"]  # its partner: same group of a looping grid, same class
    # storage orders: ascending, descending and neither, in A and in B
    for xi, xj in ((ai, aj), (bi, bj)):
        kinds = set()
        for r in range(len(xi) - 1):
            row = xj[xi[r]:xi[r + 1]]
            if len(row) >= 3:
                s = np.diff(row.astype(np.int64))
                kinds.add("up" if (s >= 0).all() else "down" if (s <= 0).all() else "mixed")
        assert kinds == {"up", "down", "mixed"}
    e = np.frexp(np.abs(np.concatenate((aa, ba))))[1]
    assert e.min() <= -15 and e.max() >= 15 and (aa < 0).any() and (aa > 0).any()


@pytest.mark.parametrize("regime", REGIMES)
def test_probing_shape(regime):
    c = cases.probing_case(regime)
    (ai, aj, aa), (bi, bj, ba) = c["A"], c["B"]
    blen = np.diff(bi)
    assert 4 < blen.mean() <= 8 and c["n"] == 2**31 - 1 and bj.max() == 2**31 - 2
    assert len(aj) * blen.mean() / c["m"] < cases.keys_max(16, regime) and c["m"] >= 64
    for T in cases.TABLES:  # one home slot for each set in every table; "last" is slot T - 1: the chain wraps
        assert set(cases.home_slot(c["last"], T).tolist()) == {T - 1}
        assert len(set(cases.home_slot(c["mid"], T).tolist())) == 1
    assert c["last"].max() > 2**31 - 2**12 and c["mid"].max() > 2**31 - 2**12  # columns near INT32_MAX
    d = distinct_per_row(c["A"], c["B"])
    for i, T in c["expect"].items():
        assert d[i] == cases.keys_max(T, regime) == blen[aj[ai[i]:ai[i + 1]]].sum()
        cols = np.unique(np.concatenate([bj[bi[k]:bi[k + 1]] for k in aj[ai[i]:ai[i + 1]]]))
        want = {"last": {T - 1}, "mid": {int(cases.home_slot(c["mid"][:1], T)[0])}}
        want["both"] = want["last"] | want["mid"]
        slots = set(cases.home_slot(cols[cols != 2**31 - 2], T).tolist())
        assert slots == want[c["slot"][i]]
    assert sorted(set(c["expect"].values())) == list(cases.TABLES)


@pytest.mark.parametrize("regime", REGIMES)
def test_too_wide_shape(regime):
    c = cases.too_wide_case(regime)
    d = distinct_per_row(c["A"], c["B"])
    assert d[c["row"]] == c["d"] == cases.keys_max(1024, regime) + 2 - (regime == "half")
    assert np.delete(d, c["row"]).max() <= 16 and c["m"] >= 64


@pytest.mark.parametrize("name", ["fits", "nine", "dense"])
def test_p0_shape(name):
    c = cases.p0_case(name)
    ai, aj, aa = c["A"]
    agg, dist = c["agg"], c["distinct"]
    assert (agg == -1).any() and agg.max() < c["na"] and c["m"] > 256
    assert (agg[aj] == -1).any()  # columns without an aggregate are named
    if name == "dense":
        assert len(aj) > 8 * c["m"]
        return
    assert len(aj) <= 8 * c["m"]
    assert {0, 1, 7, 8} <= set(dist.tolist())
    assert dist.max() == (9 if name == "nine" else 8) and np.count_nonzero(dist == 9) == (name == "nine")
    assert (np.diff(ai) > dist).any()  # several columns in one aggregate
    assert (np.diff(ai)[dist == 8] > 8).any()  # a ninth entry that is no ninth column


def test_prolong_shape():
    c = cases.prolong_case()
    ti, tj, ta = c["T"]
    kinds = set()
    for i in range(c["m"]):
        cols, g = tj[ti[i]:ti[i + 1]], c["agg"][i]
        assert (np.diff(cols) > 0).all()
        if g < 0:
            kinds.add("none-empty" if len(cols) == 0 else "none")
        elif len(cols) == 0:
            kinds.add("empty")
        elif g in cols:
            kinds.add("on")
        else:
            kinds.add("below" if g < cols[0] else "above" if g > cols[-1] else "between")
    assert kinds == {"none-empty", "none", "empty", "on", "below", "above", "between"}
    assert tj.max() == c["n"] - 1 >= c["na"] and c["agg"].max() < c["na"] and c["alpha"] < 0 and c["m"] > 256


def test_tentative_shape():
    c = cases.tentative_case()
    count = np.bincount(c["agg"][c["agg"] >= 0], minlength=c["na"])
    assert np.array_equal(count, c["sizes"]) and {0, 1, 2, 63, 64, 65, 1000} <= set(count.tolist())
    assert (c["agg"] == -1).any() and c["na"] > 256
    assert count[c["empty"]] == 0 and count[c["zero"]] > 0 and not c["B"][c["agg"] == c["zero"]].any()
    big = np.flatnonzero(c["agg"] == 5)
    assert (np.diff(big) > 1).any()  # members spread through the rows, not contiguous
    Bc, p0, s2 = ogamg.tentative_ref(c["agg"], c["B"], c["na"])
    assert Bc[c["empty"]] == 0 and Bc[c["zero"]] == 0 and not p0[c["agg"] == c["zero"]].any()
    assert not p0[c["agg"] == -1].any() and (p0[(c["agg"] >= 0) & (c["agg"] != c["zero"])] != 0).all()


def test_diagnostics_refuse_malformed_operands(pkg):
    """Checked on the host, before anything is uploaded: offsets that fall,
    columns outside B's rows, aggregates outside [-1, na)."""
    G = importlib.import_module("petsc-openacc_amd.gamg")
    ok = (np.array([0, 1], np.int32), np.array([0], np.int32), np.ones(1))
    for A, B in (((np.array([0, 2, 1], np.int32), np.array([0], np.int32), np.ones(1)), ok),
                 ((np.array([0, 1], np.int32), np.array([1], np.int32), np.ones(1)), ok),
                 (ok, (np.array([0, 1], np.int32), np.array([3], np.int32), np.ones(1)))):
        with pytest.raises(pkg.AIJHIPError) as e:
            G.device_rowprod(A, B, 2)
        assert e.value.code == pkg.AIJHIP_ERR_ARG
    for agg in ([2], [-2]):
        with pytest.raises(pkg.AIJHIPError) as e:
            G.device_rowprod_p0(ok, agg, [1.0], 2)
        assert e.value.code == pkg.AIJHIP_ERR_ARG
        with pytest.raises(pkg.AIJHIPError) as e:
            G.device_tentative(agg, [1.0], 2)
        assert e.value.code == pkg.AIJHIP_ERR_ARG
