"""KSPBCGS (AIJHIP_KSP_BCGS) without a GPU: the numpy restatement of the
specified algorithm (tests/bcgs_reference.py) against a direct solve and on
its exits, and the new boundary (header, library exports, Python binding)."""
import ctypes
import importlib
import re

import numpy as np
import pytest

import bcgs_reference as ref
from conftest import ROOT
from oracle import seqaij


def operand(pkg, N, c):
    ai, aj, aa = pkg.poisson_csr(N)
    return ai, aj, ref.convection_csr(ai, aj, aa, c)


def test_convection_operand_is_nonsymmetric_and_keeps_the_structure(pkg):
    sp = pytest.importorskip("scipy.sparse")
    ai, aj, aa0 = pkg.poisson_csr(6)
    for c in (0.3, "variable"):
        aa = ref.convection_csr(ai, aj, aa0, c)
        A = sp.csr_matrix((aa, aj, ai), shape=(216, 216))
        assert abs(A - A.T).max() > 0.0
        assert np.count_nonzero(aa) == np.count_nonzero(aa0)
    assert np.array_equal(ref.convection_csr(ai, aj, aa0, 0.0), aa0)


@pytest.mark.parametrize("pc", ["none", "jacobi"])
def test_restatement_solves_to_spsolve(pkg, pc):
    sp = pytest.importorskip("scipy.sparse")
    spla = pytest.importorskip("scipy.sparse.linalg")
    N = 8
    ai, aj, aa = operand(pkg, N, 0.3)
    b, _ = pkg.poisson_vectors(N)
    dinv = ref.jacobi_inverse(ai, aj, aa) if pc == "jacobi" else None
    x, its, reason, hist = ref.bcgs(lambda y: seqaij.matmult(ai, aj, aa, y),
                                    (lambda y: dinv * y) if pc == "jacobi" else (lambda y: y), b, rtol=1e-10)
    assert reason == ref.CONVERGED_RTOL and 0 < its <= 100 and len(hist) == its + 1
    xs = spla.spsolve(sp.csr_matrix((aa, aj, ai), shape=(N ** 3,) * 2).tocsc(), b)
    assert np.linalg.norm(x - xs) <= 1e-8 * np.linalg.norm(xs)
    assert np.linalg.norm(b - seqaij.matmult(ai, aj, aa, x)) <= 1e-8 * np.linalg.norm(b)


def test_restatement_iteration_limit(pkg):
    ai, aj, aa = operand(pkg, 8, 0.3)
    b, _ = pkg.poisson_vectors(8)
    x, its, reason, hist = ref.bcgs(lambda y: seqaij.matmult(ai, aj, aa, y), lambda y: y, b, rtol=0.0, max_it=7)
    assert reason == ref.DIVERGED_ITS and its == 7 and len(hist) == 8
    x, its, reason, hist = ref.bcgs(lambda y: seqaij.matmult(ai, aj, aa, y), lambda y: y, b, rtol=0.0, max_it=0)
    assert reason == ref.DIVERGED_ITS and its == 0 and len(hist) == 1 and not x.any()


def test_restatement_breakdown_and_exact_exit():
    A = np.array([[0.0, 1.0], [-1.0, 0.0]])
    x, its, reason, hist = ref.bcgs(lambda y: A @ y, lambda y: y, np.array([1.0, 0.0]))
    assert reason == ref.DIVERGED_BREAKDOWN and its == 0 and not x.any() and len(hist) == 1
    # 1 x 1: s = t = 0 in the first iteration, the d2 == 0 exit takes x += alpha p
    x, its, reason, hist = ref.bcgs(lambda y: 2.0 * y, lambda y: 0.5 * y, np.array([1.0]))
    assert reason == ref.CONVERGED_RTOL and its == 1 and x[0] == 0.5 and hist[-1] == 0.0


def test_header_declares_and_library_exports_the_type_calls(pkg):
    hdr = (ROOT / "include" / "aijhip_ksp.h").read_text()
    for name in ("aijhip_ksp_set_type", "aijhip_ksp_get_type"):
        assert re.search(r"^int %s\(aijhip_ksp_t" % name, hdr, re.M), name
    assert re.search(r"AIJHIP_KSP_CG = 0, AIJHIP_KSP_BCGS = 1", hdr)
    assert re.search(r"AIJHIP_KSP_DIVERGED_BREAKDOWN = -5", hdr)
    L = ctypes.CDLL(str(pkg.LIB_PATH))
    assert hasattr(L, "aijhip_ksp_set_type") and hasattr(L, "aijhip_ksp_get_type")
    K = importlib.import_module("petsc-openacc_amd.ksp")
    assert {"aijhip_ksp_set_type", "aijhip_ksp_get_type"} <= set(K.KSP_SYMBOLS)
    assert K.DIVERGED_BREAKDOWN == -5 and K.REASONS[-5] == "DIVERGED_BREAKDOWN"
    assert K.KSP_TYPES == {"cg": 0, "bcgs": 1} and issubclass(K.KSPBCGS, K.KSPCG)
    # a NULL handle is refused before any device work
    K._lib()
    assert pkg.lib().aijhip_ksp_set_type(None, 1) == pkg.AIJHIP_ERR_ARG
    assert pkg.lib().aijhip_ksp_get_type(None, None) == pkg.AIJHIP_ERR_ARG


def test_main_ksp_refuses_an_unknown_type_and_ships_the_bcgs_config(pkg):
    import subprocess
    exe = importlib.import_module("petsc-openacc_amd.build").build_main_ksp()
    r = subprocess.run([str(exe), "-ksp_type", "gmres", "-da_grid_x", "4"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "gmres not supported (cg or bcgs)" in r.stderr
    cfg = (ROOT / "configs" / "bcgs_jacobi.info").read_text()
    assert "-ksp_type bcgs" in cfg and "-pc_type jacobi" in cfg
