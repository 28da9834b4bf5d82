"""Host-side smoothed-aggregation hierarchy (include/aijhip_gamg.h), exposed
for inspection and testing; the KSP builds it itself for AIJHIP_PC_GAMG."""
from __future__ import annotations

import ctypes
import importlib

import numpy as np

_pkg = importlib.import_module("petsc-openacc_amd")

GAMG_SYMBOLS = (
    "aijhip_gamg_params_default", "aijhip_gamg_build_host", "aijhip_gamg_host_num_levels",
    "aijhip_gamg_host_level_info", "aijhip_gamg_host_get_A", "aijhip_gamg_host_get_P",
    "aijhip_gamg_host_get_aggregates", "aijhip_gamg_host_view", "aijhip_gamg_host_destroy",
    "aijhip_mg_smoother_default", "aijhip_mg_cheby_coefficients",
    "aijhip_gamg_diag_rowprod", "aijhip_gamg_diag_rowprod_p0", "aijhip_gamg_diag_prolong",
    "aijhip_gamg_diag_tentative", "aijhip_gamg_diag_info", "aijhip_gamg_diag_get_csr",
    "aijhip_gamg_diag_get_passes", "aijhip_gamg_diag_destroy",
    "aijhip_gamg_diag_rowprod_numeric", "aijhip_gamg_diag_numeric_classes",
)
SMOOTHER_TYPES = {"richardson": 0, "chebyshev": 1}


class GamgParams(ctypes.Structure):
    _fields_ = [("threshold", ctypes.c_double), ("coarse_eq_limit", ctypes.c_int32),
                ("max_levels", ctypes.c_int32), ("nsmooths", ctypes.c_int32),
                ("smooth_scale", ctypes.c_double), ("eig_its", ctypes.c_int32), ("threads", ctypes.c_int32),
                ("device_min_rows", ctypes.c_int32), ("coarsen", ctypes.c_int32), ("square_graph", ctypes.c_int32),
                ("eig_ksp", ctypes.c_int32), ("pad0", ctypes.c_int32)]


class MgSmoother(ctypes.Structure):
    """aijhip_mg_smoother_t: the V-cycle's level smoother."""
    _fields_ = [("type", ctypes.c_int32), ("its", ctypes.c_int32), ("richardson_scale", ctypes.c_double),
                ("cheby_lo", ctypes.c_double), ("cheby_hi", ctypes.c_double)]


_P = ctypes.c_void_p
_bound = False


def _lib():
    global _bound
    L = _pkg.lib()
    if not _bound:
        for n in GAMG_SYMBOLS:
            getattr(L, n).restype = ctypes.c_int
        L.aijhip_gamg_params_default.argtypes = [ctypes.POINTER(GamgParams)]
        L.aijhip_gamg_build_host.argtypes = [ctypes.c_int32, _P, _P, _P, ctypes.POINTER(GamgParams), ctypes.POINTER(_P)]
        L.aijhip_gamg_host_num_levels.argtypes = [_P, ctypes.POINTER(ctypes.c_int32)]
        L.aijhip_gamg_host_level_info.argtypes = [_P, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                                  ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64),
                                                  ctypes.POINTER(ctypes.c_double)]
        L.aijhip_gamg_host_get_A.argtypes = [_P, ctypes.c_int32, _P, _P, _P]
        L.aijhip_gamg_host_get_P.argtypes = [_P, ctypes.c_int32, _P, _P, _P]
        L.aijhip_gamg_host_get_aggregates.argtypes = [_P, ctypes.c_int32, _P]
        L.aijhip_gamg_host_destroy.argtypes = [_P]
        L.aijhip_mg_smoother_default.argtypes = [ctypes.POINTER(MgSmoother)]
        L.aijhip_mg_cheby_coefficients.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_int32,
                                                   ctypes.POINTER(ctypes.c_double), _P]
        i32, d = ctypes.c_int32, ctypes.c_double
        L.aijhip_gamg_diag_rowprod.argtypes = [i32, i32, i32, _P, _P, _P, _P, _P, _P, i32, ctypes.POINTER(_P)]
        L.aijhip_gamg_diag_rowprod_p0.argtypes = [i32, i32, i32, _P, _P, _P, _P, _P, i32, ctypes.POINTER(_P)]
        L.aijhip_gamg_diag_prolong.argtypes = [i32, i32, _P, _P, _P, _P, _P, _P, d, ctypes.POINTER(_P)]
        L.aijhip_gamg_diag_tentative.argtypes = [i32, i32, _P, _P, i32, _P, _P, _P]
        L.aijhip_gamg_diag_info.argtypes = [_P, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(ctypes.c_int64),
                                            ctypes.POINTER(i32), ctypes.POINTER(i32)]
        L.aijhip_gamg_diag_get_csr.argtypes = [_P, _P, _P, _P]
        L.aijhip_gamg_diag_get_passes.argtypes = [_P, _P, _P]
        L.aijhip_gamg_diag_destroy.argtypes = [_P]
        L.aijhip_gamg_diag_rowprod_numeric.argtypes = [i32, i32, i32, _P, _P, _P, _P, _P, _P, _P, _P, i32,
                                                       ctypes.POINTER(_P)]
        L.aijhip_gamg_diag_numeric_classes.argtypes = [_P, i32, ctypes.POINTER(i32)]
        _bound = True
    return L


def default_params(**over) -> GamgParams:
    p = GamgParams()
    _lib().aijhip_gamg_params_default(ctypes.byref(p))
    for k, v in over.items():
        setattr(p, k, v)
    return p


def mg_smoother(type="richardson", its=None, scale=None, lo=None, hi=None) -> MgSmoother:
    """aijhip_mg_smoother_default with the given fields replaced: type
    "richardson" or "chebyshev", its = steps per sweep, scale = Richardson's
    scale, lo / hi = Chebyshev's bounds as factors of the level's emax
    estimate."""
    s = MgSmoother()
    _pkg._check(_lib().aijhip_mg_smoother_default(ctypes.byref(s)))
    if type not in SMOOTHER_TYPES:
        raise ValueError(f"smoother type {type!r}: one of {sorted(SMOOTHER_TYPES)}")
    s.type = SMOOTHER_TYPES[type]
    for field, v in (("its", its), ("richardson_scale", scale), ("cheby_lo", lo), ("cheby_hi", hi)):
        if v is not None:
            setattr(s, field, v)
    return s


def cheby_coefficients(emax: float, emin: float, k: int):
    """(scale, omega[0..k)) of aijhip_mg_cheby_coefficients."""
    scale = ctypes.c_double()
    omega = np.zeros(max(int(k), 1), np.float64)
    _pkg._check(_lib().aijhip_mg_cheby_coefficients(emax, emin, int(k), ctypes.byref(scale), omega.ctypes.data))
    return scale.value, omega[: int(k)]


def build_host(ai, aj, aa, **params):
    """Returns [dict(m, A=(ai,aj,aa) for l>=1, P=(ai,aj,aa), agg, emax)] per level."""
    L = _lib()
    ai = np.ascontiguousarray(ai, dtype=np.int32)
    aj = np.ascontiguousarray(aj, dtype=np.int32)
    aa = np.ascontiguousarray(aa, dtype=np.float64)
    h = _P()
    p = default_params(**params)
    rc = L.aijhip_gamg_build_host(len(ai) - 1, ai.ctypes.data, aj.ctypes.data, aa.ctypes.data, ctypes.byref(p),
                                  ctypes.byref(h))
    if rc:
        raise _pkg.AIJHIPError(rc, "aijhip_gamg_build_host failed")
    try:
        n = ctypes.c_int32()
        L.aijhip_gamg_host_num_levels(h, ctypes.byref(n))
        out = []
        for lvl in range(n.value):
            m, na, npp, em = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_double()
            L.aijhip_gamg_host_level_info(h, lvl, ctypes.byref(m), ctypes.byref(na), ctypes.byref(npp), ctypes.byref(em))
            d = {"m": m.value, "nnz_a": na.value, "emax": em.value}
            if lvl >= 1:
                a = (np.empty(m.value + 1, np.int32), np.empty(na.value, np.int32), np.empty(na.value))
                L.aijhip_gamg_host_get_A(h, lvl, *[x.ctypes.data for x in a])
                d["A"] = a
            if lvl < n.value - 1:
                pr = (np.empty(m.value + 1, np.int32), np.empty(npp.value, np.int32), np.empty(npp.value))
                L.aijhip_gamg_host_get_P(h, lvl, *[x.ctypes.data for x in pr])
                d["P"] = pr
                agg = np.empty(m.value, np.int32)
                L.aijhip_gamg_host_get_aggregates(h, lvl, agg.ctypes.data)
                d["agg"] = agg
            out.append(d)
        return out
    finally:
        L.aijhip_gamg_host_destroy(h)


# ---- diagnostics (include/aijhip_gamg.h "Diagnostics") ----

def _csr_args(ai, aj, aa):
    ai = np.ascontiguousarray(ai, dtype=np.int32)
    aj = np.ascontiguousarray(aj, dtype=np.int32)
    aa = np.ascontiguousarray(aa, dtype=np.float64)
    if len(ai) < 1 or len(aj) != ai[-1] or len(aa) != ai[-1]:
        raise ValueError("CSR arrays do not fit each other")
    return ai, aj, aa


def _diag_result(L, rc, h):
    """(ai, aj, aa) of a diagnostic handle and what its product launched:
    dict(passes=[(lanes, table, mode, keys_max)], row_table, p0_register,
    shape). The handle is destroyed."""
    _pkg._check(rc)
    try:
        m, n, nz, npass, reg = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int32()
        _pkg._check(L.aijhip_gamg_diag_info(h, ctypes.byref(m), ctypes.byref(n), ctypes.byref(nz), ctypes.byref(npass),
                                            ctypes.byref(reg)))
        ai, aj, aa = np.empty(m.value + 1, np.int32), np.empty(nz.value, np.int32), np.empty(nz.value, np.float64)
        _pkg._check(L.aijhip_gamg_diag_get_csr(h, ai.ctypes.data, aj.ctypes.data, aa.ctypes.data))
        passes = np.empty((npass.value, 4), np.int32)
        row_table = np.empty(m.value, np.int32)
        _pkg._check(L.aijhip_gamg_diag_get_passes(h, passes.ctypes.data, row_table.ctypes.data))
        report = {"passes": [(int(g), int(t), "write" if w else "count", int(k)) for g, t, w, k in passes],
                  "row_table": row_table, "p0_register": bool(reg.value), "shape": (m.value, n.value)}
        return (ai, aj, aa), report
    finally:
        L.aijhip_gamg_diag_destroy(h)


def device_rowprod(A, B, n, n_cu=0):
    """C = A B through the device set-up's hash-table product. A, B: (ai, aj,
    aa) host CSR, A m x k, B k x n. Returns ((ci, cj, ca), report)."""
    L = _lib()
    ai, aj, aa = _csr_args(*A)
    bi, bj, ba = _csr_args(*B)
    h = _P()
    rc = L.aijhip_gamg_diag_rowprod(len(ai) - 1, len(bi) - 1, int(n), ai.ctypes.data, aj.ctypes.data, aa.ctypes.data,
                                    bi.ctypes.data, bj.ctypes.data, ba.ctypes.data, int(n_cu), ctypes.byref(h))
    return _diag_result(L, rc, h)


def device_rowprod_numeric(A, B, n, ci, cj, n_cu=0):
    """The values of C = A B on the known pattern (ci, cj ascending per row)
    through the refresh's numeric-only kernel. Returns ((ci, cj, ca), report);
    report["passes"] = [(lanes, capacity, "write", capacity)] per launch."""
    L = _lib()
    ai, aj, aa = _csr_args(*A)
    bi, bj, ba = _csr_args(*B)
    ci = np.ascontiguousarray(ci, dtype=np.int32)
    cj = np.ascontiguousarray(cj, dtype=np.int32)
    if len(ci) != len(ai) or len(cj) != ci[-1]:
        raise ValueError("the pattern does not fit A's rows")
    h = _P()
    rc = L.aijhip_gamg_diag_rowprod_numeric(len(ai) - 1, len(bi) - 1, int(n), ai.ctypes.data, aj.ctypes.data,
                                            aa.ctypes.data, bi.ctypes.data, bj.ctypes.data, ba.ctypes.data,
                                            ci.ctypes.data, cj.ctypes.data, int(n_cu), ctypes.byref(h))
    return _diag_result(L, rc, h)


def numeric_classes():
    """[(lanes, capacity)]: every instantiation of the numeric-only kernel."""
    L = _lib()
    n = ctypes.c_int32()
    _pkg._check(L.aijhip_gamg_diag_numeric_classes(None, 0, ctypes.byref(n)))
    pairs = np.zeros((max(n.value, 1), 2), np.int32)
    _pkg._check(L.aijhip_gamg_diag_numeric_classes(pairs.ctypes.data, n.value, ctypes.byref(n)))
    return [(int(g), int(c)) for g, c in pairs[: n.value]]


def device_rowprod_p0(A, agg, p0, na, n_cu=0):
    """T = A P0 through the device set-up's rowprod_p0 (P0 row j: column
    agg[j], value p0[j], empty where agg[j] = -1). A: (ai, aj, aa), m x
    len(agg). Returns ((ti, tj, ta), report)."""
    L = _lib()
    ai, aj, aa = _csr_args(*A)
    agg = np.ascontiguousarray(agg, dtype=np.int32)
    p0 = np.ascontiguousarray(p0, dtype=np.float64)
    if len(agg) != len(p0):
        raise ValueError("agg and p0 differ in length")
    h = _P()
    rc = L.aijhip_gamg_diag_rowprod_p0(len(ai) - 1, len(agg), int(na), ai.ctypes.data, aj.ctypes.data, aa.ctypes.data,
                                       agg.ctypes.data, p0.ctypes.data, int(n_cu), ctypes.byref(h))
    return _diag_result(L, rc, h)


def device_prolong(T, n, agg, p0, dinv, alpha):
    """P = P0 + alpha D^-1 T through prolong_from_T. T: (ti, tj, ta), m x n,
    ascending columns. Returns (pi, pj, pa)."""
    L = _lib()
    ti, tj, ta = _csr_args(*T)
    m = len(ti) - 1
    agg = np.ascontiguousarray(agg, dtype=np.int32)
    p0 = np.ascontiguousarray(p0, dtype=np.float64)
    dinv = np.ascontiguousarray(dinv, dtype=np.float64)
    if not (len(agg) == len(p0) == len(dinv) == m):
        raise ValueError("agg, p0 and dinv have one entry per row of T")
    h = _P()
    rc = L.aijhip_gamg_diag_prolong(m, int(n), ti.ctypes.data, tj.ctypes.data, ta.ctypes.data, agg.ctypes.data,
                                    p0.ctypes.data, dinv.ctypes.data, float(alpha), ctypes.byref(h))
    return _diag_result(L, rc, h)[0]


def device_tentative(agg, B, na, b_ones=False):
    """(Bc, p0, s2) of tentative_device and aggregate_sumsq_device."""
    L = _lib()
    agg = np.ascontiguousarray(agg, dtype=np.int32)
    B = np.ascontiguousarray(B, dtype=np.float64)
    if len(agg) != len(B):
        raise ValueError("agg and B differ in length")
    Bc, p0, s2 = np.empty(int(na)), np.empty(len(agg)), np.empty(int(na))
    rc = L.aijhip_gamg_diag_tentative(len(agg), int(na), agg.ctypes.data, B.ctypes.data, int(bool(b_ones)),
                                      Bc.ctypes.data, p0.ctypes.data, s2.ctypes.data)
    _pkg._check(rc)
    return Bc, p0, s2
