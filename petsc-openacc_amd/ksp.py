"""Device-resident CG (include/aijhip_ksp.h) — the KSP side of the path.

Mirrors the reference's solver set-up (/root/reference/src/main_ksp.cpp:92-103:
KSPCreate, KSPSetOperators, KSPSetType(KSPCG), KSPSetFromOptions, KSPSetUp,
KSPSolve, KSPGetConvergedReason / IterationNumber / ResidualNorm) over the
C ABI. Options follow /root/reference/configs/PETSc_SolverOptions_GAMG.info
(-ksp_atol 1e-12 -ksp_rtol 1e-14 -ksp_max_it 10000); the preconditioner is
Jacobi (the reference's smoother / coarse PC) until the GAMG hierarchy lands.
"""
from __future__ import annotations

import ctypes
import math
import importlib
import time

import numpy as np

_pkg = importlib.import_module("petsc-openacc_amd")

PC_TYPES = {"none": 0, "jacobi": 1, "gamg": 2, "bjacobi_gamg": 3}
NORM_TYPES = {"none": 0, "preconditioned": 1, "unpreconditioned": 2, "natural": 3}
KSP_TYPES = {"cg": 0, "bcgs": 1}
DIVERGED_BREAKDOWN = -5  # AIJHIP_KSP_DIVERGED_BREAKDOWN (BiCGStab)
REASONS = {2: "CONVERGED_RTOL", 3: "CONVERGED_ATOL", -3: "DIVERGED_ITS", -4: "DIVERGED_DTOL",
           -5: "DIVERGED_BREAKDOWN", -8:"DIVERGED_INDEFINITE_PC", -9: "DIVERGED_NANORINF", -10: "DIVERGED_INDEFINITE_MAT"}
KSP_SYMBOLS = (
    "aijhip_ksp_create", "aijhip_ksp_set_tolerances", "aijhip_ksp_set_pc_type", "aijhip_ksp_set_norm_type",
    "aijhip_ksp_set_initial_guess_nonzero", "aijhip_ksp_set_up", "aijhip_ksp_solve",
    "aijhip_ksp_get_iteration_number", "aijhip_ksp_get_residual_norm", "aijhip_ksp_get_converged_reason",
    "aijhip_ksp_get_residual_history", "aijhip_ksp_get_fused", "aijhip_ksp_destroy",
    "aijhip_ksp_set_gamg_params", "aijhip_ksp_get_pc_levels", "aijhip_ksp_get_pc_level",
    "aijhip_ksp_get_gamg_setup_path", "aijhip_ksp_get_host_syncs", "aijhip_ksp_get_iteration_bytes",
    "aijhip_ksp_solve_host", "aijhip_ksp_set_mg_smoother", "aijhip_ksp_get_mg_smoother",
    "aijhip_ksp_mat_solve", "aijhip_ksp_mat_solve_host", "aijhip_ksp_get_mat_solve_results",
    "aijhip_ksp_get_mat_solve_history", "aijhip_ksp_get_mat_solve_bytes",
    "aijhip_ksp_set_mat_vcycle_width", "aijhip_ksp_get_mat_vcycle_width", "aijhip_ksp_pc_apply",
    "aijhip_ksp_pc_mat_apply", "aijhip_ksp_set_gamg_reuse_interpolation", "aijhip_ksp_get_gamg_reuse_interpolation",
    "aijhip_ksp_get_gamg_setup_counts", "aijhip_ksp_get_mat_vcycle_reserve",
    "aijhip_ksp_set_type", "aijhip_ksp_get_type",
)
KSP_MAX_RHS = 64  # AIJHIP_KSP_MAX_RHS
_P = ctypes.c_void_p
_bound = False


def _lib():
    global _bound
    L = _pkg.lib()
    if not _bound:
        for n in KSP_SYMBOLS:
            getattr(L, n).restype = ctypes.c_int
        L.aijhip_ksp_create.argtypes = [_P, ctypes.POINTER(_P)]
        L.aijhip_ksp_set_tolerances.argtypes = [_P, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int32]
        L.aijhip_ksp_set_pc_type.argtypes = [_P, ctypes.c_int]
        L.aijhip_ksp_set_norm_type.argtypes = [_P, ctypes.c_int]
        L.aijhip_ksp_set_initial_guess_nonzero.argtypes = [_P, ctypes.c_int]
        L.aijhip_ksp_set_up.argtypes = [_P]
        L.aijhip_ksp_solve.argtypes = [_P, _P, _P, _P]
        L.aijhip_ksp_solve_host.argtypes = [_P, _P, _P]
        L.aijhip_ksp_get_iteration_number.argtypes = [_P, ctypes.POINTER(ctypes.c_int32)]
        L.aijhip_ksp_get_residual_norm.argtypes = [_P, ctypes.POINTER(ctypes.c_double)]
        L.aijhip_ksp_get_converged_reason.argtypes = [_P, ctypes.POINTER(ctypes.c_int)]
        L.aijhip_ksp_get_residual_history.argtypes = [_P, _P, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]
        L.aijhip_ksp_get_fused.argtypes = [_P, ctypes.POINTER(ctypes.c_int)]
        L.aijhip_ksp_get_host_syncs.argtypes = [_P, ctypes.POINTER(ctypes.c_int32)]
        L.aijhip_ksp_get_iteration_bytes.argtypes = [_P, ctypes.POINTER(ctypes.c_int64),
                                                     ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
        L.aijhip_ksp_destroy.argtypes = [_P]
        L.aijhip_ksp_set_gamg_params.argtypes = [_P, _P]
        L.aijhip_ksp_set_mg_smoother.argtypes = [_P, _P]
        L.aijhip_ksp_get_mg_smoother.argtypes = [_P, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                                 ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double),
                                                 ctypes.POINTER(ctypes.c_double)]
        L.aijhip_ksp_get_pc_level.argtypes = [_P, ctypes.c_int32, ctypes.c_char, ctypes.POINTER(ctypes.c_int32),
                                              ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64), _P, _P, _P]
        L.aijhip_ksp_get_pc_levels.argtypes = [_P, ctypes.POINTER(ctypes.c_int32), _P, _P, ctypes.c_int32,
                                               ctypes.POINTER(ctypes.c_double)]
        L.aijhip_ksp_get_gamg_setup_path.argtypes = [_P, ctypes.c_int32, _P, _P, ctypes.POINTER(ctypes.c_int32)]
        L.aijhip_ksp_mat_solve.argtypes = [_P, ctypes.c_int32, ctypes.c_int, _P, ctypes.c_int64, _P, ctypes.c_int64, _P]
        L.aijhip_ksp_mat_solve_host.argtypes = L.aijhip_ksp_mat_solve.argtypes[:-1]
        L.aijhip_ksp_get_mat_solve_results.argtypes = [_P, ctypes.c_int32, _P, _P, _P, ctypes.POINTER(ctypes.c_int32)]
        L.aijhip_ksp_get_mat_solve_history.argtypes = [_P, ctypes.c_int32, _P, ctypes.c_int32,
                                                       ctypes.POINTER(ctypes.c_int32)]
        L.aijhip_ksp_get_mat_solve_bytes.argtypes = [_P, ctypes.c_int32, ctypes.POINTER(ctypes.c_int64),
                                                     ctypes.POINTER(ctypes.c_int64)]
        L.aijhip_ksp_set_mat_vcycle_width.argtypes = [_P, ctypes.c_int32]
        L.aijhip_ksp_get_mat_vcycle_width.argtypes = [_P, ctypes.POINTER(ctypes.c_int32)]
        L.aijhip_ksp_pc_apply.argtypes = [_P, _P, _P, _P]
        L.aijhip_ksp_pc_mat_apply.argtypes = L.aijhip_ksp_mat_solve.argtypes
        L.aijhip_ksp_set_gamg_reuse_interpolation.argtypes = [_P, ctypes.c_int]
        L.aijhip_ksp_get_gamg_reuse_interpolation.argtypes = [_P, ctypes.POINTER(ctypes.c_int)]
        L.aijhip_ksp_get_gamg_setup_counts.argtypes = [_P, ctypes.POINTER(ctypes.c_int32),
                                                       ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)]
        L.aijhip_ksp_get_mat_vcycle_reserve.argtypes = [_P, ctypes.c_int32, _P, ctypes.POINTER(ctypes.c_int32)]
        L.aijhip_ksp_set_type.argtypes = [_P, ctypes.c_int]
        L.aijhip_ksp_get_type.argtypes = [_P, ctypes.POINTER(ctypes.c_int)]
        _bound = True
    return L


class KSPCG:
    """KSPCG on a SeqAIJHIP operator (device vectors)."""

    def __init__(self, A, rtol=1e-5, atol=1e-50, dtol=1e5, max_it=10000, pc="jacobi",
                 norm="preconditioned", guess_nonzero=False, gamg=None, smoother=None, mat_vcycle=0,
                 reuse_interpolation=False, ksp_type="cg"):
        """ksp_type: "cg" or "bcgs" (aijhip_ksp_set_type; KSPBCGS is the latter);
        gamg: aijhip_gamg_params_t fields; smoother: the GAMG level smoother,
        dict(type="richardson"|"chebyshev", its=, scale=, lo=, hi=) (gamg.mg_smoother;
        None: Richardson(1), scale 1); mat_vcycle: the widest block mat_solve and
        pc_mat_apply take with pc="gamg" (aijhip_ksp_set_mat_vcycle_width; 0: they
        refuse a GAMG handle); reuse_interpolation: -pc_gamg_reuse_interpolation, new
        values on the same structure refresh the hierarchy instead of rebuilding it
        (aijhip_ksp_set_gamg_reuse_interpolation)."""
        L = _lib()
        self.A = A
        self._h = _P()
        _pkg._check(L.aijhip_ksp_create(A._h, ctypes.byref(self._h)))
        self.set_tolerances(rtol, atol, dtol, max_it)
        _pkg._check(L.aijhip_ksp_set_pc_type(self._h, PC_TYPES[pc]))
        if gamg:
            G = importlib.import_module("petsc-openacc_amd.gamg")
            self._gp = G.default_params(**gamg)
            _pkg._check(L.aijhip_ksp_set_gamg_params(self._h, ctypes.byref(self._gp)))
        if smoother:
            G = importlib.import_module("petsc-openacc_amd.gamg")
            self._sm = G.mg_smoother(**smoother)
            _pkg._check(L.aijhip_ksp_set_mg_smoother(self._h, ctypes.byref(self._sm)))
        _pkg._check(L.aijhip_ksp_set_norm_type(self._h, NORM_TYPES[norm]))
        _pkg._check(L.aijhip_ksp_set_initial_guess_nonzero(self._h, int(guess_nonzero)))
        if mat_vcycle:
            self.set_mat_vcycle_width(mat_vcycle)
        if reuse_interpolation:
            self.reuse_interpolation = True
        if ksp_type != "cg":
            self.set_type(ksp_type)

    def set_type(self, ksp_type):
        """KSPSetType (aijhip_ksp_set_type): "cg", "bcgs" or the library's
        integer code. The PC and its set-up stay."""
        _pkg._check(_lib().aijhip_ksp_set_type(self._h, KSP_TYPES.get(ksp_type, ksp_type)))

    @property
    def ksp_type(self) -> str:
        v = ctypes.c_int()
        _pkg._check(_lib().aijhip_ksp_get_type(self._h, ctypes.byref(v)))
        return {c: n for n, c in KSP_TYPES.items()}[v.value]

    @property
    def reuse_interpolation(self) -> bool:
        v = ctypes.c_int()
        _pkg._check(_lib().aijhip_ksp_get_gamg_reuse_interpolation(self._h, ctypes.byref(v)))
        return bool(v.value)

    @reuse_interpolation.setter
    def reuse_interpolation(self, flg):
        _pkg._check(_lib().aijhip_ksp_set_gamg_reuse_interpolation(self._h, int(bool(flg))))

    def setup_counts(self):
        """(full set-ups, refreshes, seconds of the last of either) of this
        handle (aijhip_ksp_get_gamg_setup_counts)."""
        full, ref, secs = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double()
        _pkg._check(_lib().aijhip_ksp_get_gamg_setup_counts(self._h, ctypes.byref(full), ctypes.byref(ref),
                                                            ctypes.byref(secs)))
        return full.value, ref.value, secs.value

    def mat_vcycle_reserve(self):
        """Device addresses of the reserved multi-column blocks (b, x, r, w per
        level) followed by the lock-step work vectors R, Z, P
        (aijhip_ksp_get_mat_vcycle_reserve): equal tuples mean kept allocations."""
        n = ctypes.c_int32()
        L = _lib()
        _pkg._check(L.aijhip_ksp_get_mat_vcycle_reserve(self._h, 0, None, ctypes.byref(n)))
        ptrs = np.zeros(max(n.value, 1), np.uint64)
        _pkg._check(L.aijhip_ksp_get_mat_vcycle_reserve(self._h, n.value, ptrs.ctypes.data, ctypes.byref(n)))
        return tuple(int(p) for p in ptrs[: n.value])

    def set_mat_vcycle_width(self, kmax: int):
        """Reserve the multi-column V-cycle's level blocks for kmax columns (at
        set-up, or at once on a set-up handle, whose hierarchy stays)."""
        _pkg._check(_lib().aijhip_ksp_set_mat_vcycle_width(self._h, int(kmax)))

    @property
    def mat_vcycle_width(self) -> int:
        v = ctypes.c_int32()
        _pkg._check(_lib().aijhip_ksp_get_mat_vcycle_width(self._h, ctypes.byref(v)))
        return v.value

    def pc_apply(self, r, z, stream=None):
        """PCApply (aijhip_ksp_pc_apply): z = M^-1 r for the handle's PC."""
        _pkg._check(_lib().aijhip_ksp_pc_apply(self._h, _pkg._dev_ptr(r, self.A.m, "r"),
                                               _pkg._dev_ptr(z, self.A.m, "z"), _pkg._stream_handle(stream)))

    def pc_mat_apply(self, R, Z, stream=None):
        """PCMatApply (aijhip_ksp_pc_mat_apply): Z = M^-1 R for float64 GPU
        tensors of shape (m, k) in one layout, as mat_solve's B and X."""
        import torch
        for t, what in ((R, "R"), (Z, "Z")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or not t.is_cuda:
                raise TypeError(f"pc_mat_apply: {what} must be a float64 torch tensor on the GPU")
        k, layout, ldr, ldz = self._mat_solve_layout(R.shape, R.stride(), Z.shape, Z.stride())
        _pkg._check(_lib().aijhip_ksp_pc_mat_apply(self._h, k, layout, R.data_ptr(), ldr, Z.data_ptr(), ldz,
                                                   _pkg._stream_handle(stream)))

    def set_tolerances(self, rtol, atol, dtol, max_it):
        _pkg._check(_lib().aijhip_ksp_set_tolerances(self._h, rtol, atol, dtol, int(max_it)))

    def set_up(self):
        _pkg._check(_lib().aijhip_ksp_set_up(self._h))

    def solve(self, b, x, stream=None):
        _pkg._check(_lib().aijhip_ksp_solve(self._h, _pkg._dev_ptr(b, self.A.m, "b"),
                                            _pkg._dev_ptr(x, self.A.m, "x"), _pkg._stream_handle(stream)))

    def solve_host(self, b: np.ndarray, x: np.ndarray):
        """KSPSolve with host arrays (aijhip_ksp_solve_host): b up and x down
        once per solve, the solve itself on the device."""
        b = np.ascontiguousarray(b, dtype=np.float64)
        if x.dtype != np.float64 or not x.flags["C_CONTIGUOUS"] or len(x) < self.A.m or len(b) < self.A.m:
            raise TypeError("solve_host: contiguous float64 arrays of the operator's size")
        _pkg._check(_lib().aijhip_ksp_solve_host(self._h, b.ctypes.data, x.ctypes.data))

    def _mat_solve_layout(self, bshape, bstrides, xshape, xstrides):
        """(k, layout, ldb, ldx) of a mat_solve's blocks from their shapes and
        strides in elements, checked before any library call."""
        bshape, xshape = tuple(int(v) for v in bshape), tuple(int(v) for v in xshape)
        if len(bshape) != 2 or len(xshape) != 2:
            raise TypeError("mat_solve: B and X are 2-D blocks of shape (m, k)")
        if bshape != xshape or bshape[0] != self.A.m:
            raise TypeError(f"mat_solve: B is {bshape} and X is {xshape}, both must be ({self.A.m}, k)")
        k = bshape[1]
        if k > KSP_MAX_RHS:
            raise ValueError(f"mat_solve: k = {k} is above AIJHIP_KSP_MAX_RHS = {KSP_MAX_RHS}")
        if k == 0:
            return 0, 1, 1, 1
        layout, ldb, ldx = _pkg._common_dense_layout(bshape, bstrides, xshape, xstrides)
        return k, layout, ldb, ldx

    def mat_solve(self, B, X, stream=None):
        """KSPMatSolve (aijhip_ksp_mat_solve): A X = B for float64 GPU tensors
        of shape (m, k), k <= 64, the columns solved as independent CG
        recurrences in lock step (PC none / Jacobi, and GAMG on a handle made with
        mat_vcycle >= k: one multi-column V-cycle per iteration). Layout and leading
        dimensions come from the strides as in SeqAIJHIP.mat_mult; B and X take
        one layout. X is overwritten (read first with a nonzero initial guess)."""
        import torch
        for t, what in ((B, "B"), (X, "X")):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
                raise TypeError(f"mat_solve: {what} must be a float64 torch tensor on the GPU")
        k, layout, ldb, ldx = self._mat_solve_layout(B.shape, B.stride(), X.shape, X.stride())
        if not (B.is_cuda and X.is_cuda):
            raise TypeError("mat_solve: B and X must be on the GPU")
        _pkg._check(_lib().aijhip_ksp_mat_solve(self._h, k, layout, B.data_ptr(), ldb, X.data_ptr(), ldx,
                                                _pkg._stream_handle(stream)))

    def mat_solve_host(self, B: np.ndarray, X: np.ndarray):
        """KSPMatSolve with host arrays (aijhip_ksp_mat_solve_host): float64
        arrays of shape (m, k) in one order (C: interleaved, Fortran: columns)."""
        for a, what in ((B, "B"), (X, "X")):
            if not isinstance(a, np.ndarray) or a.dtype != np.float64:
                raise TypeError(f"mat_solve_host: {what} must be a float64 numpy array")
        es = B.itemsize
        k, layout, ldb, ldx = self._mat_solve_layout(B.shape, [s // es for s in B.strides], X.shape,
                                                     [s // es for s in X.strides])
        _pkg._check(_lib().aijhip_ksp_mat_solve_host(self._h, k, layout, B.ctypes.data, ldb, X.ctypes.data, ldx))

    def mat_results(self) -> list:
        """[(its, reason, rnorm)] per column of the last mat_solve."""
        k = ctypes.c_int32()
        L = _lib()
        _pkg._check(L.aijhip_ksp_get_mat_solve_results(self._h, 0, None, None, None, ctypes.byref(k)))
        its = np.zeros(max(k.value, 1), np.int32)
        reason = np.zeros(max(k.value, 1), np.intc)
        rnorm = np.zeros(max(k.value, 1), np.float64)
        _pkg._check(L.aijhip_ksp_get_mat_solve_results(self._h, k.value, its.ctypes.data, reason.ctypes.data,
                                                       rnorm.ctypes.data, ctypes.byref(k)))
        return [(int(its[j]), int(reason[j]), float(rnorm[j])) for j in range(k.value)]

    def mat_history(self, j: int) -> np.ndarray:
        """Column j's residual history of the last mat_solve."""
        n = ctypes.c_int32()
        L = _lib()
        _pkg._check(L.aijhip_ksp_get_mat_solve_history(self._h, int(j), None, 0, ctypes.byref(n)))
        its = self.mat_results()[int(j)][0]
        buf = np.empty(its + 1)
        _pkg._check(L.aijhip_ksp_get_mat_solve_history(self._h, int(j), buf.ctypes.data, len(buf), ctypes.byref(n)))
        return buf[: n.value]

    def mat_solve_bytes(self, k: int):
        """(total, MatMatMult part): compulsory HBM bytes of one lock-step
        iteration at width k on the set-up solver (aijhip_ksp_get_mat_solve_bytes)."""
        t, sp = ctypes.c_int64(), ctypes.c_int64()
        _pkg._check(_lib().aijhip_ksp_get_mat_solve_bytes(self._h, int(k), ctypes.byref(t), ctypes.byref(sp)))
        return t.value, sp.value

    @property
    def its(self) -> int:
        v = ctypes.c_int32()
        _pkg._check(_lib().aijhip_ksp_get_iteration_number(self._h, ctypes.byref(v)))
        return v.value

    @property
    def reason(self) -> int:
        v = ctypes.c_int()
        _pkg._check(_lib().aijhip_ksp_get_converged_reason(self._h, ctypes.byref(v)))
        return v.value

    @property
    def rnorm(self) -> float:
        v = ctypes.c_double()
        _pkg._check(_lib().aijhip_ksp_get_residual_norm(self._h, ctypes.byref(v)))
        return v.value

    @property
    def host_syncs(self) -> int:
        """Host synchronisations of the last solve (polls + the final read)."""
        v = ctypes.c_int32()
        _pkg._check(_lib().aijhip_ksp_get_host_syncs(self._h, ctypes.byref(v)))
        return v.value

    def iteration_bytes(self):
        """(total, SpMV part, finest-level part): compulsory HBM bytes of one
        CG iteration of the set-up solver (aijhip_ksp_get_iteration_bytes)."""
        t, sp, l0 = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _pkg._check(_lib().aijhip_ksp_get_iteration_bytes(self._h, ctypes.byref(t), ctypes.byref(sp),
                                                          ctypes.byref(l0)))
        return t.value, sp.value, l0.value

    @property
    def fused(self) -> bool:
        v = ctypes.c_int()
        _pkg._check(_lib().aijhip_ksp_get_fused(self._h, ctypes.byref(v)))
        return bool(v.value)

    def pc_levels(self):
        """(rows per level, nnz per level, host set-up seconds) of the PC."""
        n = ctypes.c_int32()
        rows = np.zeros(32, np.int32)
        nnz = np.zeros(32, np.int64)
        secs = ctypes.c_double()
        _pkg._check(_lib().aijhip_ksp_get_pc_levels(self._h, ctypes.byref(n), rows.ctypes.data, nnz.ctypes.data,
                                                     32, ctypes.byref(secs)))
        return rows[: n.value].tolist(), nnz[: n.value].tolist(), secs.value

    def mg_smoother(self, level: int):
        """(type, its, emin, emax) of the set-up PC's smoother on `level`: the
        bounds are the ones a Chebyshev level uses (0, 0 for Richardson)."""
        ty, its, lo, hi = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double(), ctypes.c_double()
        _pkg._check(_lib().aijhip_ksp_get_mg_smoother(self._h, int(level), ctypes.byref(ty), ctypes.byref(its),
                                                       ctypes.byref(lo), ctypes.byref(hi)))
        return ("richardson", "chebyshev")[ty.value], its.value, lo.value, hi.value

    def setup_path(self):
        """Per coarsening l -> l+1: ("device"|"host", widest product
        accumulator: 0 = wavefront form, 32/64/128/256 LDS columns, -1 host), and
        whether a device level overflowed to the host builder."""
        path = np.zeros(32, np.int32)
        cols = np.zeros(32, np.int32)
        fb = ctypes.c_int32()
        _pkg._check(_lib().aijhip_ksp_get_gamg_setup_path(self._h, 32, path.ctypes.data, cols.ctypes.data,
                                                           ctypes.byref(fb)))
        n = len(self.pc_levels()[0]) - 1
        return [("device" if path[l] else "host", int(cols[l])) for l in range(n)], bool(fb.value)

    def pc_level(self, l: int, which: str = "A"):
        """(ai, aj, aa, ncols) of GAMG level l's operator ('A') or
        interpolation to level l+1 ('P'), copied from the device."""
        m, n, nz = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
        L = _lib()
        _pkg._check(L.aijhip_ksp_get_pc_level(self._h, l, which.encode(), ctypes.byref(m), ctypes.byref(n),
                                              ctypes.byref(nz), None, None, None))
        ai = np.empty(m.value + 1, np.int32)
        aj = np.empty(max(nz.value, 1), np.int32)
        aa = np.empty(max(nz.value, 1), np.float64)
        _pkg._check(L.aijhip_ksp_get_pc_level(self._h, l, which.encode(), None, None, None, ai.ctypes.data,
                                              aj.ctypes.data, aa.ctypes.data))
        return ai, aj[: nz.value], aa[: nz.value], n.value

    def history(self) -> np.ndarray:
        buf = np.empty(self.its + 1)
        n = ctypes.c_int32()
        _pkg._check(_lib().aijhip_ksp_get_residual_history(self._h, buf.ctypes.data, len(buf), ctypes.byref(n)))
        return buf[: n.value]

    def destroy(self):
        if getattr(self, "_h", None) and self._h.value:
            _lib().aijhip_ksp_destroy(self._h)
            self._h = _P()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.destroy()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class KSPBCGS(KSPCG):
    """KSPBCGS on a SeqAIJHIP operator: preconditioned BiCGStab for nonsymmetric
    operators (AIJHIP_KSP_BCGS), with KSPCG's interface. mat_solve raises the
    library's error (the lock-step solver is CG); only norm="preconditioned"
    solves."""

    def __init__(self, A, *args, **kwargs):
        kwargs["ksp_type"] = "bcgs"
        super().__init__(A, *args, **kwargs)


def bench_cg(pkg, A, nx, ny, nz, dev, iters=200):
    """CG iterations/s on the device at the benchmark operand: a fixed count
    of iterations (rtol = atol = 0, so every iteration runs), timed whole."""
    import torch
    rhs, _ = pkg.poisson_vectors(nx, ny, nz)
    b = torch.from_numpy(rhs).to(dev)
    x = torch.empty_like(b)
    with KSPCG(A, rtol=0.0, atol=0.0, max_it=iters) as ksp:
        ksp.set_up()
        ksp.solve(b, x)  # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ksp.solve(b, x)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        its, fused = ksp.its, ksp.fused
        nb, nb_spmv, _ = ksp.iteration_bytes()
    return {"iters": its, "seconds": round(dt, 4), "iters_per_s": round(its / dt, 2),
            "ms_per_iter": round(dt / its * 1e3, 4), "pc": "jacobi", "fused_spmv_dot": fused,
            "bytes_per_iter": nb, "GBs": round(nb * its / dt / 1e9, 1),
            "roofline": {"bound": "hbm", "bytes_per_iter": nb, "spmv_bytes_per_iter": nb_spmv,
                         "achieved": round(nb * its / dt / 1e9, 1), "peak": 8000.0, "unit": "GB/s",
                         "frac": round(nb * its / dt / 1e9 / 8000.0, 4),
                         "note": "aijhip_ksp_get_iteration_bytes: the SpMV at its layout's bytes + the vector "
                                 "passes, per iteration, over the measured wall time of the iterations"}}


def bench_cg_gamg(pkg, A, nx, ny, nz, dev, rtol=1e-14, atol=1e-12, max_it=10000, gamg=None, light=False,
                  smoother=None):
    """The reference's solver configuration (CG + GAMG to atol 1e-12 / rtol
    1e-14, configs/cg_gamg.info) solved to convergence on the benchmark
    operand from x = 0: KSPSetUp (host hierarchy + uploads) and KSPSolve
    timed separately, the solve once warm (a second solve on the same
    hierarchy, as a time-stepping caller would). gamg: the hierarchy's
    parameters (aijhip_gamg_params_t fields); light: skip the host-vector
    solve and the second set-up; smoother: the level smoother (KSPCG's)."""
    import torch
    rhs, exact = pkg.poisson_vectors(nx, ny, nz)
    b = torch.from_numpy(rhs).to(dev)
    x = torch.zeros_like(b)
    with KSPCG(A, rtol=rtol, atol=atol, max_it=max_it, pc="gamg", gamg=gamg, smoother=smoother) as ksp:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ksp.set_up()
        torch.cuda.synchronize()
        t_setup = time.perf_counter() - t0
        rows, nnz, t_host = ksp.pc_levels()
        t0 = time.perf_counter()
        ksp.solve(b, x)
        torch.cuda.synchronize()
        t_first = time.perf_counter() - t0
        x.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ksp.solve(b, x)
        torch.cuda.synchronize()
        t_solve = time.perf_counter() - t0
        its, reason, rnorm, syncs = ksp.its, ksp.reason, ksp.rnorm, ksp.host_syncs
        nb, nb_spmv, nb_l0 = ksp.iteration_bytes()
        # the same solve from HOST b / x (aijhip_ksp_solve_host: the PETSc KSP
        # type "cghip" for an unchanged caller with host Vecs)
        t_host_solve, host_same = None, None
        if not light:
            xh = np.zeros(A.m)
            t0 = time.perf_counter()
            ksp.solve_host(rhs, xh)
            t_host_solve = time.perf_counter() - t0
            host_same = bool(np.array_equal(xh.view(np.uint64), x.cpu().numpy().view(np.uint64)))
    err = float((x.cpu() - torch.from_numpy(exact)).abs().max())
    roof = {"bound": "hbm", "bytes_per_iter": nb, "spmv_bytes_per_iter": nb_spmv,
            "finest_level_bytes_per_iter": nb_l0,
            "achieved": round(nb * its / t_solve / 1e9, 1), "peak": 8000.0, "unit": "GB/s",
            "frac": round(nb * its / t_solve / 1e9 / 8000.0, 4),
            "note": "aijhip_ksp_get_iteration_bytes (every SpMV of the hierarchy at its layout's "
                    "bytes — A_l twice, P, P^T per level — plus CG's and the V-cycle's vector passes) "
                    "x iterations / the solve's wall time (polls and launch gaps included)"}
    # the same set-up again in this process (a caller that rebuilds the
    # hierarchy after new values): the first one above also pays one-time
    # costs (the set-up kernels' first launch, pinned staging)
    with KSPCG(A, rtol=rtol, atol=atol, max_it=max_it, pc="gamg", gamg=gamg, smoother=smoother) as ksp2:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ksp2.set_up()
        torch.cuda.synchronize()
        t_again = time.perf_counter() - t0
    if light:
        return {"its": its, "reason": reason, "max_err": err, "setup_s": round(t_setup, 3),
                "setup_again_s": round(t_again, 3), "solve_s": round(t_solve, 4),
                "time_to_solution_s": round(t_setup + t_solve, 3),
                "ms_per_iter": round(t_solve / max(its, 1) * 1e3, 4),
                "levels": [{"rows": r, "nnz": z} for r, z in zip(rows, nnz)], "roofline": roof}
    return {"its": its, "reason": reason, "rnorm": rnorm, "max_err": err,
            "setup_s": round(t_setup, 3), "setup_again_s": round(t_again, 3), "setup_pc_s": round(t_host, 3),
            "solve_s": round(t_solve, 4), "first_solve_s": round(t_first, 4),
            "solve_host_vectors": {"s": round(t_host_solve, 4), "bitwise_equal_device_solve": host_same,
                                   "note": "aijhip_ksp_solve_host: b up and x down once per solve (the KSP type "
                                           "cghip of the PETSc adapter for host Vecs), PCIe included"},
            "ms_per_iter": round(t_solve / max(its, 1) * 1e3, 4), "host_syncs": syncs,
            "time_to_solution_s": round(t_setup + t_solve, 3),
            "levels": [{"rows": r, "nnz": z} for r, z in zip(rows, nnz)],
            "roofline": roof,
            "options": "cg, gamg agg nsmooths 1 threshold 0, mg levels "
                       + ("richardson(1)" if not smoother else
                          f"{smoother.get('type', 'richardson')}({smoother.get('its', 1)})")
                       + "+jacobi, coarse preonly+jacobi, rtol 1e-14 atol 1e-12"}


# ----------------------------------------------------------------------------
# Row-partitioned CG: one process per GPU, the operator an
# MPIAIJ row block (petsc-openacc_amd/mpiaij.py), every dot product a local
# fixed-order reduction on the device (include/aijhip_vec.h) combined across
# ranks by one all-reduce (RCCL over xGMI with the nccl backend) — PETSc's
# VecDot/VecNorm -> MPI_Allreduce. The iteration is KSPSolve_CG [ext] as in
# aijhip_ksp (and oracle/ksp_cg.py): the scalar decisions run on the host
# from the reduced values, which every rank holds identically, so all ranks
# take the same branch. PC: Jacobi (PETSc's bjacobi + jacobi sub-PC per rank)
# or none.

VEC_SYMBOLS = ("aijhip_vec_aypx", "aijhip_vec_dot", "aijhip_vec_cg_update", "aijhip_vec_jacobi",
               "aijhip_mat_jacobi_inverse", "aijhip_read_probe", "aijhip_delay_probe")

_vec_bound = False


def _veclib():
    global _vec_bound
    L = _pkg.lib()
    if not _vec_bound:
        for n in VEC_SYMBOLS:
            getattr(L, n).restype = ctypes.c_int
        i64, d = ctypes.c_int64, ctypes.c_double
        L.aijhip_vec_aypx.argtypes = [i64, d, _P, _P, _P]
        L.aijhip_vec_dot.argtypes = [i64, _P, _P, _P, _P]
        L.aijhip_vec_cg_update.argtypes = [i64, d, _P, _P, _P, _P, _P, _P, _P, _P]
        L.aijhip_vec_jacobi.argtypes = [i64, _P, _P, _P, _P, _P]
        L.aijhip_mat_jacobi_inverse.argtypes = [_P, _P, _P]
        L.aijhip_read_probe.argtypes = [_P, i64, ctypes.c_int, _P]
        L.aijhip_delay_probe.argtypes = [d, _P]
        _vec_bound = True
    return L


class DeviceVecOps:
    """The HIP vector kernels (aijhip_vec.h) on float64 GPU tensors; each
    reduction lands in a small device tensor ready for the all-reduce."""

    def __init__(self, device):
        import torch
        self.red = torch.zeros(3, dtype=torch.float64, device=device)

    @staticmethod
    def _s():
        import torch
        return torch.cuda.current_stream().cuda_stream

    def aypx(self, beta, x, y):
        _pkg._check(_veclib().aijhip_vec_aypx(x.numel(), beta, x.data_ptr(), y.data_ptr(), self._s()))

    def dot(self, x, y):
        _pkg._check(_veclib().aijhip_vec_dot(x.numel(), x.data_ptr(), y.data_ptr(), self.red.data_ptr(), self._s()))
        return self.red[:1]

    def cg_update(self, a, x, p, r, w, z, dinv):
        _pkg._check(_veclib().aijhip_vec_cg_update(x.numel(), a, x.data_ptr(), p.data_ptr(), r.data_ptr(),
                                                   w.data_ptr(), z.data_ptr(),
                                                   dinv.data_ptr() if dinv is not None else None,
                                                   self.red.data_ptr(), self._s()))
        return self.red

    def jacobi(self, r, dinv, z):
        _pkg._check(_veclib().aijhip_vec_jacobi(r.numel(), r.data_ptr(), dinv.data_ptr() if dinv is not None else None,
                                                z.data_ptr(), self.red.data_ptr(), self._s()))
        return self.red

    @staticmethod
    def jacobi_inverse(A_diag, dinv):
        _pkg._check(_veclib().aijhip_mat_jacobi_inverse(A_diag._h, dinv.data_ptr(), DeviceVecOps._s()))


class KSPCGMPI:
    """KSPSolve_CG over a row-partitioned operator. op: object with
    mult(x, y) on this rank's rows (MPIAIJ); dinv: this rank's Jacobi inverse
    (None = PCNONE); ops: vector backend (DeviceVecOps on the GPU)."""

    CONVERGED_RTOL, CONVERGED_ATOL = 2, 3
    DIVERGED_ITS, DIVERGED_DTOL, DIVERGED_INDEFINITE_PC, DIVERGED_NANORINF, DIVERGED_INDEFINITE_MAT = \
        -3, -4, -8, -9, -10

    def __init__(self, op, mloc, dinv=None, ops=None, rtol=1e-5, atol=1e-50, dtol=1e5, max_it=10000,
                 norm="preconditioned", group=None, device=None):
        import torch
        self.op, self.m, self.dinv = op, mloc, dinv
        self.ops = ops if ops is not None else DeviceVecOps(device)
        self.rtol, self.atol, self.dtol, self.max_it, self.norm = rtol, atol, dtol, max_it, norm
        self.group = group
        dev = device if device is not None else (dinv.device if dinv is not None else None)
        mk = lambda: torch.zeros(mloc, dtype=torch.float64, device=dev)  # noqa: E731
        self.r, self.z, self.p = mk(), mk(), mk()
        self.its, self.reason, self.rnorm, self.hist = 0, 0, 0.0, []

    def _allreduce(self, t):
        """Sum over ranks (in place) and return the values on the host."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1:
            dist.all_reduce(t, group=self.group)
        return [float(v) for v in t.tolist()]

    def _norm(self, zz, zr, rr):
        if self.norm == "preconditioned":
            return math.sqrt(zz)
        if self.norm == "unpreconditioned":
            return math.sqrt(rr)
        return math.sqrt(abs(zr))

    def _test(self, rn):
        if math.isnan(rn) or math.isinf(rn):
            return self.DIVERGED_NANORINF
        if rn <= self.ttol:
            return self.CONVERGED_ATOL if rn < self.atol else self.CONVERGED_RTOL
        if rn >= self.dtol * self.rnorm0:
            return self.DIVERGED_DTOL
        return 0

    def solve(self, b, x):
        """Zero initial guess (main_ksp.cpp: VecSet(lhs, 0))."""
        ops, r, z, p = self.ops, self.r, self.z, self.p
        x.zero_()
        r.copy_(b)
        zz, zr, rr = self._allreduce(ops.jacobi(r, self.dinv, z))
        dp = self._norm(zz, zr, rr)
        self.hist = [dp]
        self.rnorm0 = dp
        self.ttol = max(self.rtol * dp, self.atol)
        self.reason = self._test(dp)
        self.its, self.rnorm = 0, dp
        if self.reason:
            return self.reason
        beta, betaold, dpi = zr, 0.0, 0.0
        i = 0
        while i < self.max_it:
            self.its = i + 1
            if beta == 0.0:
                self.reason = self.CONVERGED_ATOL
                return self.reason
            if i > 0 and beta * betaold < 0.0:
                self.reason = self.DIVERGED_INDEFINITE_PC
                return self.reason
            if i == 0:
                p.copy_(z)
            else:
                ops.aypx(beta / betaold, z, p)
            self.op.mult(p, z)  # W = A P (W shares Z's storage)
            dpiold, dpi = dpi, self._allreduce(ops.dot(p, z))[0]
            betaold = beta
            if dpi == 0.0 or (i > 0 and dpi * dpiold <= 0.0):
                self.reason = self.DIVERGED_INDEFINITE_MAT
                return self.reason
            a = beta / dpi
            zz, zr, rr = self._allreduce(ops.cg_update(a, x, p, r, z, z, self.dinv))
            dp = self._norm(zz, zr, rr)
            self.hist.append(dp)
            self.rnorm = dp
            self.reason = self._test(dp)
            if self.reason:
                return self.reason
            beta = zr
            i += 1
        self.reason = self.DIVERGED_ITS
        return self.reason
