"""The GAMG level smoothers on the GPU: CG preconditioned by the V-cycle with
Richardson(k) / Chebyshev(k) + Jacobi (csrc/mg_cycle.hip; the fused steps are
OpMgPost / OpMgCheby launches of csrc/aijhip_kernels.hip) against oracle CG
with the numpy restatement of tests/test_mg_smoothers.py.

The bars are tests/test_gamg.py::test_gpu_cg_gamg_matches_oracle's: the same
reason, iterations +-1, the first 10 history norms to rtol 1e-7, the solution
to 1e-8 relative."""
import importlib
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT
from oracle import gamg as ogamg
from test_mg_smoothers import TOL, oracle_cg, poisson_levels, poisson_oracle
from test_row_patterns_gpu import assert_bits
from test_templates_solver_gpu import LAYOUTS, OPERANDS

gpu = pytest.mark.gpu

torch = pytest.importorskip("torch")

CHEBY = {k: dict(type="chebyshev", its=k) for k in (1, 2, 3)}
SMOOTHERS = {"chebyshev1": CHEBY[1], "chebyshev2": CHEBY[2], "chebyshev3": CHEBY[3],
             "richardson2": dict(type="richardson", its=2),
             "richardson2-scale2/3": dict(type="richardson", its=2, scale=2.0 / 3.0)}
RICHARDSON1 = dict(type="richardson", its=1)
_cache = {}


@pytest.fixture(autouse=True)
def _plain_env(monkeypatch):
    monkeypatch.delenv("AIJHIP_KSP_EXPLICIT_Z", raising=False)
    monkeypatch.delenv("AIJHIP_MG_UNFUSED", raising=False)


def solve(pkg, csr, rhs, smoother, layout=None):
    """One CG + GAMG solve from x = 0 (the environment is read at set-up):
    dict(its, reason, hist, x, rows, bytes, smoothers per smoothed level)."""
    K = importlib.import_module("petsc-openacc_amd.ksp")
    ai, aj, aa = csr
    b = torch.from_numpy(rhs).cuda()
    x = torch.zeros_like(b)
    with pkg.SeqAIJHIP(ai, aj, aa, **(LAYOUTS[layout] if layout else {})) as A:
        with K.KSPCG(A, pc="gamg", smoother=smoother, **TOL) as ksp:
            ksp.set_up()
            ksp.solve(b, x)
            torch.cuda.synchronize()
            rows = ksp.pc_levels()[0]
            return dict(its=ksp.its, reason=ksp.reason, hist=np.array(ksp.history()), x=x.cpu().numpy(), rows=rows,
                        bytes=ksp.iteration_bytes(), info=A.info(),
                        smoothers=[ksp.mg_smoother(l) for l in range(len(rows) - 1)])


def poisson_solve(pkg, N, smoother):
    """The N^3 reference problem in the default environment, once per smoother."""
    key = (N, None if smoother is None else tuple(sorted(smoother.items())))
    if key not in _cache:
        _cache[key] = solve(pkg, pkg.poisson_csr(N), pkg.poisson_vectors(N)[0], smoother)
    return _cache[key]


def assert_meets_oracle(got, ref):
    xo, its_o, reason_o, hist_o = ref
    print(f"its {got['its']} (oracle {its_o}), reason {got['reason']} ({reason_o})")
    assert got["reason"] == reason_o, (got["reason"], reason_o)
    assert abs(got["its"] - its_o) <= 1, (got["its"], its_o)
    k = min(10, len(got["hist"]), len(hist_o))
    np.testing.assert_allclose(got["hist"][:k], hist_o[:k], rtol=1e-7)
    assert np.linalg.norm(got["x"] - xo) <= 1e-8 * np.linalg.norm(xo)


def assert_same_bits(a, b):
    assert (a["its"], a["reason"]) == (b["its"], b["reason"])
    assert len(a["hist"]) == len(b["hist"])
    assert_bits(a["hist"], b["hist"])
    assert_bits(a["x"], b["x"])


@gpu
@pytest.mark.parametrize("name", list(SMOOTHERS))
@pytest.mark.parametrize("N", [12, 24])
def test_poisson_matches_the_restated_vcycle(pkg, N, name):
    """3 levels at 12^3, 4 at 24^3 (the finest on the pipelined row templates);
    odd and even step counts take the two buffer rotations."""
    levels = poisson_levels(N)[5]
    assert len(levels) == (3 if N == 12 else 4)
    got = poisson_solve(pkg, N, SMOOTHERS[name])
    assert got["rows"] == [L["A"].shape[0] for L in levels]
    assert_meets_oracle(got, poisson_oracle(N, SMOOTHERS[name]))


@gpu
def test_richardson3_iterations_at_24(pkg):
    sm = dict(type="richardson", its=3)
    got, ref = poisson_solve(pkg, 24, sm), poisson_oracle(24, sm)
    assert got["reason"] == ref[2] == 3 and abs(got["its"] - ref[1]) <= 1, (got["its"], ref[1])


@gpu
def test_chebyshev_takes_fewer_iterations_and_reports_its_bounds(pkg):
    N = 24
    cheby, rich = poisson_solve(pkg, N, CHEBY[1]), poisson_solve(pkg, N, RICHARDSON1)
    print(f"its: chebyshev(1) {cheby['its']}, richardson(1) {rich['its']}")
    assert cheby["its"] < rich["its"]  # the CPU oracle: 21 against 48
    levels = poisson_levels(N)[5]
    assert len(cheby["smoothers"]) == len(levels) - 1
    for (ty, its, emin, emax), L in zip(cheby["smoothers"], levels):
        assert (ty, its) == ("chebyshev", 1)
        assert abs(emin - 0.05 * L["emax"]) <= 1e-12 * 0.05 * L["emax"]
        assert abs(emax - 1.05 * L["emax"]) <= 1e-12 * 1.05 * L["emax"]
    custom = solve(pkg, pkg.poisson_csr(12), pkg.poisson_vectors(12)[0], dict(type="chebyshev", its=2, lo=0.1, hi=1.2))
    for (ty, its, emin, emax), L in zip(custom["smoothers"], poisson_levels(12)[5]):
        assert (ty, its) == ("chebyshev", 2)
        assert abs(emin - 0.1 * L["emax"]) <= 1e-12 * L["emax"] and abs(emax - 1.2 * L["emax"]) <= 1e-12 * L["emax"]
    assert all(s == ("richardson", 1, 0.0, 0.0) for s in rich["smoothers"])


LAYOUT_OPERANDS = ("paired7-3blocks", "paired7-22blocks", "paired7-empty-rows", "hub-chain-1500", "box9-40x37",
                   "box9-90x83")
CPU_ITS = {"chebyshev1": (18, 20), "chebyshev2": (12, 15), "richardson1": (23, 27)}


def layout_operand(name):
    """(csr, rhs = A (standard normal), oracle hierarchy)."""
    if ("op", name) not in _cache:
        ai, aj, aa = OPERANDS[name][0]()
        m = len(ai) - 1
        Asp = sp.csr_matrix((aa, aj, ai), shape=(m, m))
        rhs = Asp @ np.random.default_rng(7).standard_normal(m)
        _cache["op", name] = ((ai, aj, aa), rhs, ogamg.build(Asp, coarse_eq_limit=50))
    return _cache["op", name]


def layout_oracle(name, smname, sm):
    if ("oracle", name, smname) not in _cache:
        (ai, aj, aa), rhs, levels = layout_operand(name)
        _cache["oracle", name, smname] = oracle_cg(ai, aj, aa, rhs, levels, sm)
    return _cache["oracle", name, smname]


@pytest.mark.parametrize("name", LAYOUT_OPERANDS)
def test_layout_operands_converge_on_the_cpu(name):
    """Every operand of the layout test converges with the restated V-cycle,
    in the iteration ranges the GPU runs are then held to (+-1)."""
    for smname, sm in (("chebyshev1", CHEBY[1]), ("chebyshev2", CHEBY[2]), ("richardson1", RICHARDSON1)):
        _, its, reason, _ = layout_oracle(name, smname, sm)
        lo, hi = CPU_ITS[smname]
        assert reason == 3 and lo <= its <= hi, (name, smname, its, reason)


@gpu
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("name", LAYOUT_OPERANDS)
def test_chebyshev_bitwise_across_layouts(pkg, monkeypatch, name, k):
    """The 7- and 8-slot pipelined template kernels, the form without a
    diagonal slot, the 2-rows-per-lane kernel and grids with odd per-XCD block
    counts: iterations, history and solution equal bit for bit on aj, row
    patterns and row templates, and with AIJHIP_KSP_EXPLICIT_Z=1; and they
    meet the CPU restatement."""
    csr, rhs, _ = layout_operand(name)
    runs = {layout: solve(pkg, csr, rhs, CHEBY[k], layout) for layout in LAYOUTS}
    for layout, r in runs.items():
        assert r["info"]["row_templates"] == (layout == "templates")
        assert (r["info"]["row_patterns"] > 0) == (layout != "aj")
    for layout in ("patterns", "templates"):
        assert_same_bits(runs[layout], runs["aj"])
    monkeypatch.setenv("AIJHIP_KSP_EXPLICIT_Z", "1")
    assert_same_bits(solve(pkg, csr, rhs, CHEBY[k], "templates"), runs["templates"])
    assert_meets_oracle(runs["templates"], layout_oracle(name, f"chebyshev{k}", CHEBY[k]))


@gpu
def test_chebyshev_fused_against_unfused(pkg, monkeypatch):
    """AIJHIP_MG_UNFUSED=1 (MatMult, then the elementwise step) at
    test_gpu_vcycle_fused_smoothers_bitwise's bars: the same iterations, the
    histories to 1e-12."""
    N = 24
    fused = poisson_solve(pkg, N, CHEBY[2])
    monkeypatch.setenv("AIJHIP_MG_UNFUSED", "1")
    unfused = solve(pkg, pkg.poisson_csr(N), pkg.poisson_vectors(N)[0], CHEBY[2])
    assert unfused["its"] == fused["its"]
    np.testing.assert_allclose(unfused["hist"], fused["hist"], rtol=1e-12, atol=1e-15 * fused["hist"][0])
    np.testing.assert_allclose(unfused["x"], fused["x"], rtol=1e-10, atol=1e-12 * np.abs(fused["x"]).max())


@gpu
def test_defaults_untouched_and_bytes_counted(pkg):
    """No smoother and Richardson(1) are one code path: the same iterations,
    history bits, solution bits and bytes per iteration. Chebyshev(1) adds,
    per smoothed level, two products of A_l at its layout's bytes (the
    finest operand's own info; a coarse level's from a handle on its CSR) and the row
    operands of the fused steps: (8 + D) m down (b, D^-1) and (16 + D) m up
    (b, D^-1, p_km1), D = 1 where D^-1 is read through a template id, else 8
    (include/aijhip_ksp.h)."""
    K = importlib.import_module("petsc-openacc_amd.ksp")
    N = 24
    none, rich, cheby = poisson_solve(pkg, N, None), poisson_solve(pkg, N, RICHARDSON1), poisson_solve(pkg, N, CHEBY[1])
    assert_same_bits(none, rich)
    assert none["bytes"] == rich["bytes"]
    ai, aj, aa = pkg.poisson_csr(N)
    added = added_l0 = 0
    with pkg.SeqAIJHIP(ai, aj, aa) as A, K.KSPCG(A, pc="gamg", smoother=CHEBY[1], **TOL) as ksp:
        ksp.set_up()
        rows, nnz, _ = ksp.pc_levels()
        for l in range(len(rows) - 1):
            if l == 0:
                info = A.info()
                la, D = info["mult_layout_bytes"], 1 if info["row_templates"] else 8
            else:  # a coarse operator: a handle of its own on the same CSR takes the same plan
                lai, laj, laa, _ = ksp.pc_level(l, "A")
                assert (len(lai) - 1, lai[-1]) == (rows[l], nnz[l])
                with pkg.SeqAIJHIP(lai, laj, laa) as Al:
                    la, D = Al.info()["mult_layout_bytes"], 8
            print(f"level {l}: {rows[l]} rows, {nnz[l]} entries, {la} bytes per product, D = {D}")
            add = 2 * la + ((8 + D) + (16 + D)) * rows[l]
            added += add
            added_l0 += add if l == 0 else 0
    print(f"bytes per iteration: richardson(1) {rich['bytes']}, chebyshev(1) {cheby['bytes']}, expected + {added}")
    assert cheby["bytes"][0] == rich["bytes"][0] + added
    assert cheby["bytes"][2] == rich["bytes"][2] + added_l0


@gpu
def test_setter_clears_the_set_up_and_chebyshev_needs_an_estimate(pkg):
    """A smoother set after set-up takes effect at the next solve (as new GAMG
    parameters do); NULL puts the default back; Chebyshev on a hierarchy
    without prolongator smoothing (nsmooths = 0: no emax estimate) is refused
    at set-up with AIJHIP_ERR_ARG and a message that says why."""
    import ctypes
    K = importlib.import_module("petsc-openacc_amd.ksp")
    G = importlib.import_module("petsc-openacc_amd.gamg")
    N = 12
    b = torch.from_numpy(pkg.poisson_vectors(N)[0]).cuda()
    with pkg.SeqAIJHIP(*pkg.poisson_csr(N)) as A:
        with K.KSPCG(A, pc="gamg", **TOL) as ksp:
            its = []
            for sm in (None, G.mg_smoother(**CHEBY[1]), None):
                pkg._check(K._lib().aijhip_ksp_set_mg_smoother(ksp._h, ctypes.byref(sm) if sm else None))
                x = torch.zeros_like(b)
                ksp.solve(b, x)
                torch.cuda.synchronize()
                its.append((ksp.its, ksp.mg_smoother(0)[0]))
            assert its[0] == its[2] == (poisson_solve(pkg, N, None)["its"], "richardson")
            assert its[1] == (poisson_solve(pkg, N, CHEBY[1])["its"], "chebyshev")
            bad = G.mg_smoother(type="chebyshev", its=17)
            assert K._lib().aijhip_ksp_set_mg_smoother(ksp._h, ctypes.byref(bad)) == pkg.AIJHIP_ERR_ARG
            assert ksp.mg_smoother(0)[0] == "richardson"  # a refused request changes nothing
        with K.KSPCG(A, pc="gamg", gamg=dict(nsmooths=0), smoother=CHEBY[1], **TOL) as ksp:
            with pytest.raises(pkg.AIJHIPError) as e:
                ksp.set_up()
            assert e.value.code == pkg.AIJHIP_ERR_ARG and "nsmooths" in str(e.value)


@gpu
def test_distributed_handle_takes_the_smoother():
    """One rank: KSPCGMPINative with Chebyshev(1) is the single-GPU KSPCG bit
    for bit (tests/test_solver_parity_gpu.py). Two z slabs over the host
    transport, fused and AIJHIP_MG_UNFUSED=1: the distributed hierarchy with
    the same smoother converges in the single-GPU iterations +-1, the solution
    to 1e-8 relative."""
    W = importlib.import_module("mg_smoothers_worker")
    N = 16
    one = W.run(1, N, CHEBY[1])[0]
    single = one["single"]
    assert single["smoother"][:2] == ("chebyshev", 1)
    assert (one["its"], one["reason"]) == (single["its"], single["reason"]) and single["reason"] > 0
    assert_bits(one["hist"], single["hist"])
    assert_bits(one["x"], single["x"])
    assert abs(single["its"] - poisson_oracle(N, CHEBY[1])[1]) <= 1
    for env in ({}, {"AIJHIP_MG_UNFUSED": "1"}):
        two = W.run(2, N, CHEBY[1], env)
        assert two[0]["its"] == two[1]["its"] and two[0]["reason"] == two[1]["reason"] == single["reason"]
        print(f"2 ranks {env}: its {two[0]['its']} (single GPU {single['its']}), levels {two[0]['rows']}")
        assert abs(two[0]["its"] - single["its"]) <= 1
        x = np.concatenate([two[r]["x"] for r in range(2)])
        assert np.linalg.norm(x - single["x"]) <= 1e-8 * np.linalg.norm(single["x"])


BLOCK = re.compile(r"Number of iterations: (\d+)\n" r"L2 norm of final residual: (\S+)\n"
                   r"Maximum norm of error: (\S+)\n")


@gpu
def test_driver_cheby_options_file(pkg):
    """main_ksp -config configs/cg_gamg_cheby.info at 20^3 (the pattern of
    tests/test_main_ksp.py::test_driver_cg_gamg_options_file)."""
    exe = importlib.import_module("petsc-openacc_amd.build").build_main_ksp()
    N = 20
    r = subprocess.run([str(exe), "-config", str(ROOT / "configs" / "cg_gamg_cheby.info"), "-da_grid_x", str(N),
                        "-da_grid_y", str(N), "-da_grid_z", str(N), "-aijhip_iteration_bytes"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    m = BLOCK.search(r.stdout)
    assert m and "Bytes per iteration" in r.stdout, r.stdout
    its, linf = int(m.group(1)), float(m.group(3))
    exact = poisson_levels(N)[4]
    x, its_o, reason, _ = poisson_oracle(N, CHEBY[1])
    its_r = poisson_oracle(N, RICHARDSON1)[1]
    assert reason > 0 and abs(its - its_o) <= 1, (its, its_o)
    assert its < its_r
    assert abs(linf - np.max(np.abs(x - exact))) < 1e-6  # printed with %f
