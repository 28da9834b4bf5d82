"""GAMG reuse-interpolation, the parts that need no device: the new entry
points are declared, exported and bound, refuse NULL handles, and a C99
program calls them. The refresh itself is tests/test_gamg_refresh_gpu.py, its
product kernel tests/test_gamg_refresh_products_gpu.py.

The flag's getter and setter are exercised here on NULL handles only: a KSP
handle needs a matrix handle, and aijhip_mat_create refuses to make one
without a visible device, so the round trip on a live handle (default off,
set, read back, cleared) is in the GPU file (refresh_case and
test_flag_off_rebuilds_and_flag_on_keeps_the_interpolation)."""
import ctypes
import importlib
import inspect
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW_KSP = ("aijhip_ksp_set_gamg_reuse_interpolation", "aijhip_ksp_get_gamg_reuse_interpolation",
           "aijhip_ksp_get_gamg_setup_counts", "aijhip_ksp_get_mat_vcycle_reserve")
NEW_GAMG = ("aijhip_gamg_diag_rowprod_numeric", "aijhip_gamg_diag_numeric_classes")


def mods():
    return (importlib.import_module("petsc-openacc_amd.ksp"), importlib.import_module("petsc-openacc_amd.gamg"))


def test_ctypes_signatures(pkg):
    K, G = mods()
    L, P = K._lib(), ctypes.c_void_p
    G._lib()
    pkg.lib()
    assert set(NEW_KSP) <= set(K.KSP_SYMBOLS) and set(NEW_GAMG) <= set(G.GAMG_SYMBOLS)
    assert "aijhip_mat_update_values_device" in pkg.ABI_SYMBOLS
    i32p, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    assert L.aijhip_ksp_set_gamg_reuse_interpolation.argtypes == [P, ctypes.c_int]
    assert L.aijhip_ksp_get_gamg_reuse_interpolation.argtypes == [P, ctypes.POINTER(ctypes.c_int)]
    assert L.aijhip_ksp_get_gamg_setup_counts.argtypes == [P, i32p, i32p, dp]
    assert L.aijhip_mat_update_values_device.argtypes == [P, P]
    assert L.aijhip_ksp_get_mat_vcycle_reserve.argtypes == [P, ctypes.c_int32, P, i32p]
    i32 = ctypes.c_int32
    assert L.aijhip_gamg_diag_rowprod_numeric.argtypes == [i32, i32, i32] + [P] * 8 + [i32, ctypes.POINTER(P)]
    assert L.aijhip_gamg_diag_numeric_classes.argtypes == [P, i32, i32p]
    for n in NEW_KSP + NEW_GAMG + ("aijhip_mat_update_values_device",):
        assert getattr(L, n).restype == ctypes.c_int
    # the binding's surface
    sig = inspect.signature(K.KSPCG.__init__)
    assert sig.parameters["reuse_interpolation"].default is False
    assert isinstance(K.KSPCG.reuse_interpolation, property) and K.KSPCG.reuse_interpolation.fset
    assert callable(K.KSPCG.mat_vcycle_reserve)
    assert callable(K.KSPCG.setup_counts) and callable(pkg.SeqAIJHIP.update_values_device)
    assert callable(G.device_rowprod_numeric) and callable(G.numeric_classes)


def test_abi_version_is_unchanged(pkg):
    assert pkg.lib().aijhip_abi_version() == 5


def test_null_handles_are_refused(pkg):
    K, G = mods()
    L = K._lib()
    G._lib()
    flg, full, ref, secs = ctypes.c_int(7), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double()
    assert L.aijhip_ksp_set_gamg_reuse_interpolation(None, 1) == pkg.AIJHIP_ERR_ARG
    assert b"NULL" in L.aijhip_last_error()
    assert L.aijhip_ksp_get_gamg_reuse_interpolation(None, ctypes.byref(flg)) == pkg.AIJHIP_ERR_ARG
    assert flg.value == 7
    assert L.aijhip_ksp_get_gamg_setup_counts(None, ctypes.byref(full), ctypes.byref(ref),
                                              ctypes.byref(secs)) == pkg.AIJHIP_ERR_ARG
    assert L.aijhip_ksp_get_mat_vcycle_reserve(None, 0, None, ctypes.byref(full)) == pkg.AIJHIP_ERR_ARG
    assert L.aijhip_mat_update_values_device(None, None) == pkg.AIJHIP_ERR_ARG
    assert b"NULL" in L.aijhip_last_error()
    # the diagnostics: a NULL out, and malformed operands, before any device call
    one = np.zeros(1, np.int32)
    assert L.aijhip_gamg_diag_rowprod_numeric(0, 0, 0, one.ctypes.data, None, None, one.ctypes.data, None, None,
                                              one.ctypes.data, None, 0, None) == pkg.AIJHIP_ERR_ARG
    h = ctypes.c_void_p()
    assert L.aijhip_gamg_diag_rowprod_numeric(0, 0, 0, None, None, None, None, None, None, None, None, 0,
                                              ctypes.byref(h)) == pkg.AIJHIP_ERR_ARG
    assert not h.value
    bad = np.array([1], np.int32)  # a pattern whose offsets do not start at 0
    assert L.aijhip_gamg_diag_rowprod_numeric(0, 0, 0, one.ctypes.data, None, None, one.ctypes.data, None, None,
                                              bad.ctypes.data, None, 0, ctypes.byref(h)) == pkg.AIJHIP_ERR_ARG
    assert L.aijhip_gamg_diag_numeric_classes(None, 0, None) == pkg.AIJHIP_ERR_ARG
    assert L.aijhip_gamg_diag_numeric_classes(None, 4, ctypes.byref(full)) == pkg.AIJHIP_ERR_ARG


def test_numeric_classes_cover_the_hash_product(pkg):
    """The instantiations are listed without a device: lanes within one
    wavefront, the capacities reach the hash product's 1023 columns, and both
    of a row's LDS arrays (4 + 8 bytes per column) fit 64 KiB for one group."""
    _, G = mods()
    pairs = G.numeric_classes()
    assert len(pairs) == len(set(pairs)) > 0
    for lanes, cap in pairs:
        assert lanes in (1, 2, 4, 8, 16, 32, 64) and 12 * cap <= 65536
    assert max(cap for _, cap in pairs) >= 1023
    # a short count is honoured
    n = ctypes.c_int32()
    two = np.full(6, -1, np.int32)
    assert G._lib().aijhip_gamg_diag_numeric_classes(two.ctypes.data, 2, ctypes.byref(n)) == 0
    assert n.value == len(pairs) and two[4:].tolist() == [-1, -1] and tuple(two[:2]) == pairs[0]


def test_c99_program_links_the_new_entry_points(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    hdrs = sorted(p.name for p in (ROOT / "include").glob("*.h"))
    src = tmp_path / "refresh.c"
    src.write_text("".join(f'#include "{h}"\n' for h in hdrs) + """
#include <stdio.h>
int main(void) {
    int flg = -1;
    int32_t full = -1, refreshed = -1, n = 0, pairs[64];
    double secs = -1.0;
    aijhip_gamg_diag_t d = 0;
    int bad = 0;
    bad += aijhip_ksp_set_gamg_reuse_interpolation(0, 1) != AIJHIP_ERR_ARG;
    bad += aijhip_ksp_get_gamg_reuse_interpolation(0, &flg) != AIJHIP_ERR_ARG;
    bad += aijhip_ksp_get_gamg_setup_counts(0, &full, &refreshed, &secs) != AIJHIP_ERR_ARG;
    bad += aijhip_mat_update_values_device(0, 0) != AIJHIP_ERR_ARG;
    bad += aijhip_ksp_get_mat_vcycle_reserve(0, 0, (uint64_t *)0, &n) != AIJHIP_ERR_ARG;
    bad += aijhip_gamg_diag_rowprod_numeric(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, &d) != AIJHIP_ERR_ARG;
    bad += aijhip_gamg_diag_numeric_classes(pairs, 32, &n) != AIJHIP_OK;
    printf("%d %d %d\\n", aijhip_abi_version(), bad, n > 0);
    return bad;
}
""")
    exe = tmp_path / "refresh"
    lib = importlib.import_module("petsc-openacc_amd").LIB_PATH
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", f"-I{ROOT / 'include'}",
                        str(src), "-o", str(exe), f"-L{lib.parent}", "-laijhip", f"-Wl,-rpath,{lib.parent}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split() == ["5", "0", "1"], (out.stdout, out.stderr)
