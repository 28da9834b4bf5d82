"""A numpy restatement of the preconditioned BiCGStab that include/aijhip_ksp.h
specifies for AIJHIP_KSP_BCGS (PETSc 3.7.6 KSPSolve_BCGS with left
preconditioning, KSPConvergedDefault on the preconditioned norm), and the
convection-diffusion operands its tests share. Checker only."""
from __future__ import annotations

import math

import numpy as np

CONVERGED_RTOL, CONVERGED_ATOL = 2, 3
DIVERGED_ITS, DIVERGED_DTOL, DIVERGED_BREAKDOWN, DIVERGED_NANORINF = -3, -4, -5, -9


def bcgs(mult, pc, b, x0=None, rtol=1e-5, atol=1e-50, dtol=1e5, max_it=10000):
    """Solve A x = b. mult(y) = A y and pc(y) = B^-1 y are callables on float64
    arrays (each returns a new array). x0: a nonzero initial guess. Returns
    (x, its, reason, hist) with hist[k] the preconditioned residual norm
    after k iterations."""
    b = np.asarray(b, dtype=np.float64)
    K = lambda y: pc(mult(y))  # noqa: E731
    state = {}

    def converged(n, rnorm, snorm=None):
        if n == 0:
            state["rnorm0"] = snorm
            state["ttol"] = max(rtol * snorm, atol)
        if math.isnan(rnorm) or math.isinf(rnorm):
            return DIVERGED_NANORINF
        if rnorm <= state["ttol"]:
            return CONVERGED_ATOL if rnorm < atol else CONVERGED_RTOL
        if rnorm >= dtol * state["rnorm0"]:
            return DIVERGED_DTOL
        return 0

    if x0 is None:
        x = np.zeros_like(b)
        r = pc(b.copy())
    else:
        x = np.array(x0, dtype=np.float64)
        r = pc(b - mult(x))
    dp = float(np.sqrt(r @ r))
    hist = [dp]
    its = 0
    snorm = dp if x0 is None else float(np.sqrt(np.sum(pc(b.copy()) ** 2)))
    reason = converged(0, dp, snorm)
    if reason:
        return x, its, reason, np.array(hist)
    if max_it <= 0:
        return x, its, DIVERGED_ITS, np.array(hist)
    rp = r.copy()
    rhoold = alpha = omegaold = 1.0
    p = np.zeros_like(b)
    v = np.zeros_like(b)
    i = 0
    while True:
        rho = float(r @ rp)
        beta = (rho / rhoold) * (alpha / omegaold)
        p = r - (omegaold * beta) * v + beta * p
        v = K(p)
        d1 = float(v @ rp)
        if d1 == 0.0:
            return x, its, DIVERGED_BREAKDOWN, np.array(hist)
        alpha = rho / d1
        s = r - alpha * v
        t = K(s)
        d1 = float(s @ t)
        d2 = float(t @ t)
        if d2 == 0.0:
            if float(s @ s) != 0.0:
                return x, its, DIVERGED_BREAKDOWN, np.array(hist)
            x = x + alpha * p
            its += 1
            hist.append(0.0)
            return x, its, CONVERGED_RTOL, np.array(hist)
        omega = d1 / d2
        x = x + alpha * p + omega * s
        r = s - omega * t
        dp = float(np.sqrt(r @ r))
        rhoold, omegaold = rho, omega
        its += 1
        hist.append(dp)
        reason = converged(i + 1, dp)
        if reason:
            return x, its, reason, np.array(hist)
        if rho == 0.0:
            return x, its, DIVERGED_BREAKDOWN, np.array(hist)
        i += 1
        if i >= max_it:
            return x, its, DIVERGED_ITS, np.array(hist)


def convection_csr(ai, aj, aa, c):
    """The Poisson CSR with every entry of column row - 1 multiplied by
    (1 + c) and every entry of column row + 1 by (1 - c). c: a number
    ("constant": the operator stays on row templates), or "variable": drawn
    per row from default_rng(1).uniform(0, 0.5)."""
    ai = np.asarray(ai)
    aj = np.asarray(aj)
    m = len(ai) - 1
    rows = np.repeat(np.arange(m), np.diff(ai))
    cr = np.random.default_rng(1).uniform(0, 0.5, m) if isinstance(c, str) else np.full(m, float(c))
    out = np.array(aa, dtype=np.float64)
    lo, hi = aj == rows - 1, aj == rows + 1
    out[lo] *= 1.0 + cr[rows[lo]]
    out[hi] *= 1.0 - cr[rows[hi]]
    return out


def jacobi_inverse(ai, aj, aa):
    """PCSetUp_Jacobi: the reciprocal of each row's first stored diagonal
    entry, 1 where there is none or it is 0."""
    m = len(ai) - 1
    d = np.zeros(m)
    for r in range(m):
        for k in range(ai[r], ai[r + 1]):
            if aj[k] == r:
                d[r] = aa[k]
                break
    d[d == 0.0] = 1.0
    return 1.0 / d
