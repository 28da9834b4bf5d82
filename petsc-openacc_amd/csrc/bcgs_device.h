// bcgs_device.h — KSPSolve_BCGS's device-side scalar state, scalar steps and
// vector kernels, launched by the BiCGStab driver (bcgs_solve.hip). Not part
// of the ABI.
//
// The scalar steps restate PETSc 3.7.6 KSPSolve_BCGS [ext]
// (src/ksp/ksp/impls/bcgs/bcgs.c) with left preconditioning and
// KSPConvergedDefault [ext] (cg_device.h's converged). The reductions are
// cg_device.h's: partials per block through bsum, summed by reduce_parts in
// its fixed order, so a solve is deterministic run to run.
#pragma once

#include "cg_device.h"

struct BCGSState {
    double rho, rhoold, alpha, omega, omegaold, beta, dp, rnorm0, ttol;
    int32_t its, i, reason, done;
    int32_t xpend;  // the d2 == 0 exit: its X += alpha P is not applied yet
};

namespace {

// KSPConvergedDefault on BCGSState's rnorm0 / ttol (cg_device.h's function).
__device__ int32_t bcgs_converged(int n, double rnorm, double snorm, BCGSState *S, const CGParams &p) {
    CGState c{};
    c.rnorm0 = S->rnorm0;
    c.ttol = S->ttol;
    const int32_t reason = converged(n, rnorm, snorm, &c, p);
    S->rnorm0 = c.rnorm0;
    S->ttol = c.ttol;
    return reason;
}

// GAMG, nonzero initial guess: w = b - A x (w holds A x on entry), the
// V-cycle's input.
__global__ __launch_bounds__(kVecThreads) void kb_resid(int64_t n, const double *__restrict__ b, double *w) {
    GRID_STRIDE(i, n) w[i] = b[i] + (-1.0) * w[i];
}

// Initial residual. Jacobi / none: r = D^-1 (b - A x) (w holds A x with a
// nonzero guess) and, for snorm, D^-1 b; GAMG: r came from the V-cycle and
// sb = V-cycle(b) (nonzero guess only). rp = r, p = v = 0; partials r.r
// (slot 0) and sb.sb (slot 1).
__global__ __launch_bounds__(kVecThreads) void kb_init(int64_t n, const double *__restrict__ b,
                                                       const double *__restrict__ w,
                                                       const double *__restrict__ sb,
                                                       const double *__restrict__ dinv, double *r, double *rp,
                                                       double *p, double *v, double *part, CGParams prm) {
    __shared__ double scratch[kVecThreads / 64];
    const bool jac = prm.pc == AIJHIP_PC_JACOBI, gamg = prm.pc == AIJHIP_PC_GAMG;
    double rr = 0.0, ss = 0.0;
    GRID_STRIDE(i, n) {
        double ri;
        if (gamg) {
            ri = r[i];
            if (!prm.guess_zero) { const double si = sb[i]; ss += si * si; }
        } else {
            const double bi = b[i];
            const double ui = prm.guess_zero ? bi : bi + (-1.0) * w[i];
            ri = jac ? dinv[i] * ui : ui;
            r[i] = ri;
            if (!prm.guess_zero) { const double si = jac ? dinv[i] * bi : bi; ss += si * si; }
        }
        rp[i] = ri;
        p[i] = 0.0;
        v[i] = 0.0;
        rr += ri * ri;
    }
    const int nb = gridDim.x;
    double s;
    s = bsum<kVecThreads>(rr, scratch); if (threadIdx.x == 0) part[0 * nb + blockIdx.x] = s;
    s = bsum<kVecThreads>(ss, scratch); if (threadIdx.x == 0) part[1 * nb + blockIdx.x] = s;
}

// dp = |r|, the n = 0 convergence test, max_it = 0, and the first
// iteration's scalars: rho = r.rp = |r|^2 (rp = r), rhoold = alpha =
// omegaold = 1, hence beta = rho.
__global__ __launch_bounds__(kRedThreads) void kb_step_init(const double *part, int nb, BCGSState *S, double *hist,
                                                            CGParams p) {
    __shared__ double scratch[kRedThreads / 64];
    const double rr = reduce_parts(part + 0 * nb, nb, scratch);
    const double ss = reduce_parts(part + 1 * nb, nb, scratch);
    if (threadIdx.x != 0) return;
    BCGSState s{};
    s.dp = sqrt(rr);
    hist[0] = s.dp;
    s.reason = bcgs_converged(0, s.dp, p.guess_zero ? s.dp : sqrt(ss), &s, p);
    if (!s.reason && p.max_it <= 0) s.reason = AIJHIP_KSP_DIVERGED_ITS;
    s.rho = rr;
    s.rhoold = s.alpha = s.omegaold = 1.0;
    s.omega = 0.0;
    s.beta = (s.rho / s.rhoold) * (s.alpha / s.omegaold);
    s.done = s.reason != 0;
    *S = s;
}

// K1: p = r - (omegaold beta) v + beta p.
template <bool NT>
__global__ __launch_bounds__(kVecThreads) void kb_p(int64_t n, const double *__restrict__ r,
                                                    const double *__restrict__ v, double *p, const BCGSState *S) {
    if (S->done) return;
    const double beta = S->beta, ob = S->omegaold * S->beta;
    GRID_STRIDE(i, n) vst<NT>(p + i, (r[i] - ob * v[i]) + beta * p[i]);
}

// K2 / K4: u holds A y (Jacobi / none) or V-cycle(A y) (GAMG). Jacobi:
// u = D^-1 u in place. Partials u.c (slot 0) and, with ALL (K4: u = t, c = s),
// u.u (slot 1) and c.c (slot 2).
template <bool NT, bool ALL>
__global__ __launch_bounds__(kVecThreads) void kb_pcdot(int64_t n, double *u, const double *__restrict__ dinv,
                                                        const double *__restrict__ c, double *part,
                                                        const BCGSState *S, int pc) {
    __shared__ double scratch[kVecThreads / 64];
    if (S->done) return;
    const bool jac = pc == AIJHIP_PC_JACOBI;
    double uc = 0.0, uu = 0.0, cc = 0.0;
    GRID_STRIDE(i, n) {
        double ui = u[i];
        if (jac) {  // PCApply_Jacobi
            ui = dinv[i] * ui;
            vst<NT>(u + i, ui);
        }
        const double ci = c[i];
        uc += ui * ci;
        if (ALL) {
            uu += ui * ui;
            cc += ci * ci;
        }
    }
    const int nb = gridDim.x;
    double s;
    s = bsum<kVecThreads>(uc, scratch); if (threadIdx.x == 0) part[0 * nb + blockIdx.x] = s;
    if (ALL) {
        s = bsum<kVecThreads>(uu, scratch); if (threadIdx.x == 0) part[1 * nb + blockIdx.x] = s;
        s = bsum<kVecThreads>(cc, scratch); if (threadIdx.x == 0) part[2 * nb + blockIdx.x] = s;
    }
}

// d1 = v.rp; d1 == 0: DIVERGED_BREAKDOWN (x untouched by this iteration);
// alpha = rho / d1.
__global__ __launch_bounds__(kRedThreads) void kb_step_alpha(const double *part, int nb, BCGSState *S) {
    __shared__ double scratch[kRedThreads / 64];
    if (S->done) return;
    const double d1 = reduce_parts(part, nb, scratch);
    if (threadIdx.x != 0) return;
    if (d1 == 0.0) {
        S->reason = AIJHIP_KSP_DIVERGED_BREAKDOWN;
        S->done = 1;
        return;
    }
    S->alpha = S->rho / d1;
}

// K3: s = r - alpha v.
template <bool NT>
__global__ __launch_bounds__(kVecThreads) void kb_s(int64_t n, const double *__restrict__ r,
                                                    const double *__restrict__ v, double *s, const BCGSState *S) {
    if (S->done) return;
    const double alpha = S->alpha;
    GRID_STRIDE(i, n) vst<NT>(s + i, r[i] - alpha * v[i]);
}

// d1 = s.t, d2 = t.t. d2 == 0: s != 0 is a breakdown, s == 0 the exact
// solution x + alpha p (applied by kb_final_x); else omega = d1 / d2.
__global__ __launch_bounds__(kRedThreads) void kb_step_omega(const double *part, int nb, BCGSState *S,
                                                             double *hist) {
    __shared__ double scratch[kRedThreads / 64];
    if (S->done) return;
    const double d1 = reduce_parts(part + 0 * nb, nb, scratch);
    const double d2 = reduce_parts(part + 1 * nb, nb, scratch);
    const double ss = reduce_parts(part + 2 * nb, nb, scratch);
    if (threadIdx.x != 0) return;
    if (d2 == 0.0) {
        if (ss != 0.0) {
            S->reason = AIJHIP_KSP_DIVERGED_BREAKDOWN;
        } else {
            S->xpend = 1;
            S->its += 1;
            S->dp = 0.0;
            hist[S->its] = 0.0;
            S->reason = AIJHIP_KSP_CONVERGED_RTOL;
        }
        S->done = 1;
        return;
    }
    S->omega = d1 / d2;
}

// K5: x += alpha p + omega s, r = s - omega t; partials r.r (slot 0) and
// r.rp (slot 1: the next iteration's rho).
template <bool NT>
__global__ __launch_bounds__(kVecThreads) void kb_update(int64_t n, double *x, const double *__restrict__ p,
                                                         const double *__restrict__ s,
                                                         const double *__restrict__ t,
                                                         const double *__restrict__ rp, double *r, double *part,
                                                         const BCGSState *S) {
    __shared__ double scratch[kVecThreads / 64];
    if (S->done) return;
    const double alpha = S->alpha, omega = S->omega;
    double rr = 0.0, rrp = 0.0;
    GRID_STRIDE(i, n) {
        const double si = s[i];
        vst<NT>(x + i, (x[i] + alpha * p[i]) + omega * si);
        const double ri = si - omega * t[i];
        vst<NT>(r + i, ri);
        rr += ri * ri;
        rrp += ri * rp[i];
    }
    const int nb = gridDim.x;
    double v;
    v = bsum<kVecThreads>(rr, scratch); if (threadIdx.x == 0) part[0 * nb + blockIdx.x] = v;
    v = bsum<kVecThreads>(rrp, scratch); if (threadIdx.x == 0) part[1 * nb + blockIdx.x] = v;
}

// dp = |r|, the convergence test at n = i + 1, the rho == 0 breakdown, the
// iteration limit, then the next iteration's rho = r.rp and beta.
__global__ __launch_bounds__(kRedThreads) void kb_step_iter(const double *part, int nb, BCGSState *S, double *hist,
                                                            CGParams p) {
    __shared__ double scratch[kRedThreads / 64];
    if (S->done) return;
    const double rr = reduce_parts(part + 0 * nb, nb, scratch);
    const double rrp = reduce_parts(part + 1 * nb, nb, scratch);
    if (threadIdx.x != 0) return;
    BCGSState s = *S;
    s.dp = sqrt(rr);
    s.rhoold = s.rho;
    s.omegaold = s.omega;
    s.its += 1;
    hist[s.its] = s.dp;
    s.reason = bcgs_converged(s.i + 1, s.dp, 0.0, &s, p);
    if (!s.reason && s.rho == 0.0) s.reason = AIJHIP_KSP_DIVERGED_BREAKDOWN;
    if (!s.reason) {
        s.i += 1;
        if (s.i >= p.max_it) s.reason = AIJHIP_KSP_DIVERGED_ITS;
    }
    if (!s.reason) {
        s.rho = rrp;
        s.beta = (s.rho / s.rhoold) * (s.alpha / s.omegaold);
    }
    s.done = s.reason != 0;
    *S = s;
}

// After the loop: x += alpha p of the d2 == 0 exit.
__global__ __launch_bounds__(kVecThreads) void kb_final_x(int64_t n, const double *__restrict__ p, double *x,
                                                          const BCGSState *S) {
    if (!S->xpend) return;
    const double alpha = S->alpha;
    GRID_STRIDE(i, n) x[i] = x[i] + alpha * p[i];
}

}  // namespace
