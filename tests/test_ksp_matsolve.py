"""KSPMatSolve (aijhip_ksp_mat_solve, KSPCG.mat_solve): the parts that need no
device — the entry points exist and are declared, a NULL handle is refused
with a message before any device work, and the Python wrapper checks shapes,
layouts and the width before it calls the library."""
import ctypes
import importlib
import re
import types

import numpy as np
import pytest

from conftest import ROOT

NEW = ("aijhip_ksp_mat_solve", "aijhip_ksp_mat_solve_host", "aijhip_ksp_get_mat_solve_results",
       "aijhip_ksp_get_mat_solve_history", "aijhip_ksp_get_mat_solve_bytes")


@pytest.fixture(scope="module")
def ksp(pkg):
    return importlib.import_module("petsc-openacc_amd.ksp")


def test_symbols_exported_and_declared(pkg, ksp):
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "aijhip_ksp.h").read_text(), flags=re.S)
    lib = ctypes.CDLL(str(pkg.LIB_PATH))
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in ksp.KSP_SYMBOLS
    m = re.search(r"#define\s+AIJHIP_KSP_MAX_RHS\s+(\d+)", header)
    assert m and int(m.group(1)) == 64 == ksp.KSP_MAX_RHS
    assert pkg.lib().aijhip_abi_version() == 5


def test_null_handle(pkg, ksp):
    """All five calls refuse a NULL handle before any device work."""
    L = ksp._lib()
    b, x = np.zeros(4), np.zeros(4)
    k, n, nb = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
    calls = (
        lambda: L.aijhip_ksp_mat_solve(None, 1, 1, b.ctypes.data, 1, x.ctypes.data, 1, None),
        lambda: L.aijhip_ksp_mat_solve_host(None, 1, 0, b.ctypes.data, 4, x.ctypes.data, 4),
        lambda: L.aijhip_ksp_get_mat_solve_results(None, 0, None, None, None, ctypes.byref(k)),
        lambda: L.aijhip_ksp_get_mat_solve_history(None, 0, None, 0, ctypes.byref(n)),
        lambda: L.aijhip_ksp_get_mat_solve_bytes(None, 1, ctypes.byref(nb), None),
    )
    for call in calls:
        pkg.lib().aijhip_mat_mat_mult_chunk_widths(-1, None, 0, None)  # another message in between
        assert call() == pkg.AIJHIP_ERR_ARG
        assert b"NULL" in pkg.lib().aijhip_last_error()


def handleless(ksp, m):
    """A KSPCG with no library handle: any library call it made would fail
    with an AIJHIPError, so a TypeError / ValueError came from the wrapper."""
    K = ksp.KSPCG.__new__(ksp.KSPCG)
    K.A = types.SimpleNamespace(m=m)
    K._h = ctypes.c_void_p()
    return K


def test_wrapper_rejects_mismatched_shapes(pkg, ksp):
    K = handleless(ksp, 11)
    with pytest.raises(TypeError):
        K.mat_solve_host(np.zeros((11, 3)), np.zeros((11, 4)))
    with pytest.raises(TypeError):
        K.mat_solve_host(np.zeros((10, 3)), np.zeros((10, 3)))  # not the operator's rows
    with pytest.raises(TypeError):
        K.mat_solve_host(np.zeros(11), np.zeros(11))
    with pytest.raises(TypeError):
        K.mat_solve_host(np.zeros((11, 3), np.float32), np.zeros((11, 3), np.float32))
    torch = pytest.importorskip("torch")
    with pytest.raises(TypeError):
        K.mat_solve(torch.zeros(11, 3, dtype=torch.float64), torch.zeros(11, 4, dtype=torch.float64))
    with pytest.raises(TypeError):
        K.mat_solve(np.zeros((11, 3)), np.zeros((11, 3)))


def test_wrapper_rejects_mixed_layouts(pkg, ksp):
    K = handleless(ksp, 11)
    with pytest.raises(TypeError):
        K.mat_solve_host(np.zeros((11, 4)), np.zeros((11, 4), order="F"))
    with pytest.raises(TypeError):
        K.mat_solve_host(np.zeros((22, 8))[::2, ::2], np.zeros((11, 4)))  # strided along both axes
    torch = pytest.importorskip("torch")
    with pytest.raises(TypeError):
        K.mat_solve(torch.zeros(11, 4, dtype=torch.float64), torch.zeros(4, 11, dtype=torch.float64).t())


def test_wrapper_rejects_too_many_columns(pkg, ksp):
    K = handleless(ksp, 5)
    k = ksp.KSP_MAX_RHS + 1
    with pytest.raises(ValueError):
        K.mat_solve_host(np.zeros((5, k)), np.zeros((5, k)))
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError):
        K.mat_solve(torch.zeros(5, k, dtype=torch.float64), torch.zeros(5, k, dtype=torch.float64))


def test_wrapper_reads_layout_and_leading_dimensions(pkg, ksp):
    K = handleless(ksp, 11)
    es = 8
    c, cp = np.zeros((11, 4)), np.zeros((11, 5))[:, :4]
    assert K._mat_solve_layout(c.shape, [s // es for s in c.strides], cp.shape, [s // es for s in cp.strides]) == \
        (4, pkg.DENSE_LAYOUTS["interleaved"], 4, 5)
    f, fp = np.zeros((11, 4), order="F"), np.zeros((14, 4), order="F")[:11, :]
    assert K._mat_solve_layout(f.shape, [s // es for s in f.strides], fp.shape, [s // es for s in fp.strides]) == \
        (4, pkg.DENSE_LAYOUTS["columns"], 11, 14)
