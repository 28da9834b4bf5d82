"""KSPMatSolve with GAMG, the parts that need no device: the reserved V-cycle
width and PCApply / PCMatApply are declared, exported and listed for the
bindings, refuse NULL and out-of-range arguments before any device work, and
KSPCG defaults to no reserved width."""
import ctypes
import importlib
import inspect
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("aijhip_ksp_set_mat_vcycle_width", "aijhip_ksp_get_mat_vcycle_width", "aijhip_ksp_pc_apply",
       "aijhip_ksp_pc_mat_apply")


@pytest.fixture(scope="module")
def ksp(pkg):
    return importlib.import_module("petsc-openacc_amd.ksp")


def test_symbols_exported_declared_and_listed(pkg, ksp):
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "aijhip_ksp.h").read_text(), flags=re.S)
    lib = ctypes.CDLL(str(pkg.LIB_PATH))
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in ksp.KSP_SYMBOLS
    assert pkg.lib().aijhip_abi_version() == 5  # additions only


def test_null_and_out_of_range_arguments(pkg, ksp):
    L = ksp._lib()
    r, z = np.zeros(4), np.zeros(4)
    v = ctypes.c_int32(7)
    calls = (
        (lambda: L.aijhip_ksp_set_mat_vcycle_width(None, 4), b"NULL"),
        (lambda: L.aijhip_ksp_set_mat_vcycle_width(None, -1), b"outside 0..64"),
        (lambda: L.aijhip_ksp_set_mat_vcycle_width(None, ksp.KSP_MAX_RHS + 1), b"outside 0..64"),
        (lambda: L.aijhip_ksp_get_mat_vcycle_width(None, ctypes.byref(v)), b"NULL"),
        (lambda: L.aijhip_ksp_pc_apply(None, r.ctypes.data, z.ctypes.data, None), b"NULL"),
        (lambda: L.aijhip_ksp_pc_mat_apply(None, 1, 1, r.ctypes.data, 1, z.ctypes.data, 1, None), b"NULL"),
        (lambda: L.aijhip_ksp_pc_mat_apply(None, -1, 1, r.ctypes.data, 1, z.ctypes.data, 1, None), b"NULL"),
    )
    for call, word in calls:
        pkg.lib().aijhip_mat_mat_mult_chunk_widths(-1, None, 0, None)  # another message in between
        assert call() == pkg.AIJHIP_ERR_ARG
        assert word in pkg.lib().aijhip_last_error(), pkg.lib().aijhip_last_error()
    assert v.value == 7 and not z.any()


def test_kspcg_defaults_to_no_reserved_width(ksp):
    sig = inspect.signature(ksp.KSPCG.__init__)
    assert sig.parameters["mat_vcycle"].default == 0
    for name in ("pc_apply", "pc_mat_apply", "set_mat_vcycle_width", "mat_vcycle_width"):
        assert hasattr(ksp.KSPCG, name), name
    assert "mat_vcycle" in ksp.KSPCG.mat_solve.__doc__
