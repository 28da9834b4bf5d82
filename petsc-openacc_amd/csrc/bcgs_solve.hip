// bcgs_solve.hip — device-resident preconditioned BiCGStab on the CG driver's
// operator interface (cg_solve.h).
//
// Restates PETSc 3.7.6 KSPSolve_BCGS [ext] (src/ksp/ksp/impls/bcgs/bcgs.c)
// with left preconditioning, K(y) = B^-1 (A y), and KSPConvergedDefault [ext]
// on the preconditioned residual norm. Per iteration:
//
//   K1  P = R - (omegaold beta) V + beta P
//   V = K(P): the product (CGOperator::apply_stop), then
//   K2  Jacobi: V = D^-1 V in place; the V.RP partials   [GAMG: the V-cycle first]
//   S1  scalar step: d1 = V.RP, breakdown check, alpha = rho / d1
//   K3  S = R - alpha V
//   T = K(S): the product, then
//   K4  Jacobi: T = D^-1 T in place; the S.T, T.T, S.S partials   [GAMG: V-cycle first]
//   S2  scalar step: d2 = 0 exits, omega = d1 / d2
//   K5  X += alpha P + omega S, R = S - omega T; the R.R, R.RP partials
//   S3  scalar step: dp, KSPConvergedDefault, rho = 0 check, the iteration
//       limit, the next rho = R.RP and beta
//
// R, P and the GAMG product's output W are the CG driver's vectors (W is
// CG's Z); RP, V, S, T are BCGSWork's. All scalars live on the device; every
// kernel returns at once once the device flag `done` is set, so the host
// launches iterations in batches and polls, as cg_solve does.
//
// One deliberate difference from PETSc: max_it = 0 stops with DIVERGED_ITS at
// iteration 0, as this library's CG does (PETSc's do-while would run one).
#include "bcgs_solve.h"

#include <algorithm>

void bcgs_free(BCGSWork &bw) {
    hipFree(bw.d_rp); hipFree(bw.d_v); hipFree(bw.d_s); hipFree(bw.d_t); hipFree(bw.d_state);
    if (bw.h_state) hipHostFree(bw.h_state);
    bw.d_rp = bw.d_v = bw.d_s = bw.d_t = nullptr;
    bw.d_state = bw.h_state = nullptr;
    bw.m = -1;
}

int bcgs_reserve(BCGSWork &bw, int64_t m) {
    if (bw.m == m) return AIJHIP_OK;
    bcgs_free(bw);
    const size_t vb = sizeof(double) * (size_t)std::max<int64_t>(m, 1);
    hipError_t e;
    if ((e = hipMalloc(&bw.d_rp, vb)) != hipSuccess || (e = hipMalloc(&bw.d_v, vb)) != hipSuccess ||
        (e = hipMalloc(&bw.d_s, vb)) != hipSuccess || (e = hipMalloc(&bw.d_t, vb)) != hipSuccess ||
        (e = hipMalloc(&bw.d_state, sizeof(BCGSState))) != hipSuccess ||
        (e = hipHostMalloc(&bw.h_state, sizeof(BCGSState), hipHostMallocDefault)) != hipSuccess) {
        bcgs_free(bw);
        return cg_hip(e, "KSPSetUp_BCGS allocation");
    }
    bw.m = m;
    return AIJHIP_OK;
}

namespace {

// u = K(y) without the diagonal scaling: the product under the stop flag
// into u (Jacobi / none; K2 / K4 scale it in place) or into W with the
// V-cycle W -> u after it (GAMG).
int bcgs_k(CGSolve &cg, BCGSWork &bw, CGOperator &op, const double *y, double *u, hipStream_t st) {
    const int *stop = &bw.d_state->done;
    int rc;
    if (!op.vcycle) return op.apply_stop(y, u, st, stop);
    if ((rc = op.apply_stop(y, cg.d_z, st, stop))) return rc;
    return op.pc_apply(cg.d_z, u, st, stop, nullptr, nullptr);
}

}  // namespace

int bcgs_iteration(CGSolve &cg, BCGSWork &bw, CGOperator &op, double *x, const CGParams &p, hipStream_t st) {
    const int64_t m = cg.m;
    const dim3 vg(cg.vec_grid), vt(kVecThreads), rt(kRedThreads);
    const int nb = cg.vec_grid;
    BCGSState *S = bw.d_state;
    int rc;
    hipLaunchKernelGGL(kb_p<true>, vg, vt, 0, st, m, cg.d_r, bw.d_v, cg.d_p, S);
    if ((rc = bcgs_k(cg, bw, op, cg.d_p, bw.d_v, st))) return rc;
    hipLaunchKernelGGL((kb_pcdot<true, false>), vg, vt, 0, st, m, bw.d_v, cg.d_dinv, bw.d_rp, cg.d_part, S, p.pc);
    hipLaunchKernelGGL(kb_step_alpha, dim3(1), rt, 0, st, cg.d_part, nb, S);
    hipLaunchKernelGGL(kb_s<true>, vg, vt, 0, st, m, cg.d_r, bw.d_v, bw.d_s, S);
    if ((rc = bcgs_k(cg, bw, op, bw.d_s, bw.d_t, st))) return rc;
    hipLaunchKernelGGL((kb_pcdot<true, true>), vg, vt, 0, st, m, bw.d_t, cg.d_dinv, bw.d_s, cg.d_part, S, p.pc);
    hipLaunchKernelGGL(kb_step_omega, dim3(1), rt, 0, st, cg.d_part, nb, S, cg.d_hist);
    hipLaunchKernelGGL(kb_update<true>, vg, vt, 0, st, m, x, cg.d_p, bw.d_s, bw.d_t, bw.d_rp, cg.d_r, cg.d_part, S);
    hipLaunchKernelGGL(kb_step_iter, dim3(1), rt, 0, st, cg.d_part, nb, S, cg.d_hist, p);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? AIJHIP_OK : cg_hip(e, "KSPSolve_BCGS iteration");
}

int bcgs_solve(CGSolve &cg, BCGSWork &bw, CGOperator &op, const double *b, double *x, hipStream_t s) {
    const int64_t m = cg.m;
    if (op.multi) return cg_fail(AIJHIP_ERR_STATE, "BiCGStab serves one rank");
    if (bw.m != m) return cg_fail(AIJHIP_ERR_STATE, "BiCGStab's work vectors are not reserved");
    if (m > 0 && (!b || !x)) return cg_fail(AIJHIP_ERR_ARG, "NULL vector");
    if (b == x) return cg_fail(AIJHIP_ERR_ARG, "b and x alias");
    const CGParams p{cg.rtol, cg.abstol, cg.dtol, cg.max_it, cg.normtype, cg.guess_nonzero ? 0 : 1, cg.pc};
    const dim3 vg(cg.vec_grid), vt(kVecThreads), rt(kRedThreads);
    hipError_t e = hipSuccess;
    int rc;
    // KSPSolve [ext]: zero initial guess -> x = 0; else W = A x first.
    if (!cg.guess_nonzero) {
        if (m > 0 && (e = hipMemsetAsync(x, 0, sizeof(double) * (size_t)m, s)) != hipSuccess)
            return cg_hip(e, "KSPSolve_BCGS init");
    } else if ((rc = op.apply(x, cg.d_z, s, nullptr, nullptr))) {
        return rc;
    }
    // r = B^-1 (b - A x), snorm = |B^-1 b| with a nonzero guess (no stop flag
    // yet: the device state is initialised by the first scalar step)
    const double *sb = nullptr;
    if (op.vcycle) {
        const double *rin = b;
        if (cg.guess_nonzero) {
            hipLaunchKernelGGL(kb_resid, vg, vt, 0, s, m, b, cg.d_z);
            rin = cg.d_z;
            if ((rc = op.pc_apply(b, bw.d_t, s, nullptr, nullptr, nullptr))) return rc;
            sb = bw.d_t;
        }
        if ((rc = op.pc_apply(rin, cg.d_r, s, nullptr, nullptr, nullptr))) return rc;
    }
    hipLaunchKernelGGL(kb_init, vg, vt, 0, s, m, b, cg.d_z, sb, cg.d_dinv, cg.d_r, bw.d_rp, cg.d_p, bw.d_v, cg.d_part,
                       p);
    hipLaunchKernelGGL(kb_step_init, dim3(1), rt, 0, s, cg.d_part, cg.vec_grid, bw.d_state, cg.d_hist, p);
    if ((e = hipGetLastError()) != hipSuccess) return cg_hip(e, "KSPSolve_BCGS init");
    // iterations in batches between polls
    int32_t launched = 0;
    cg.waits = 0;
    for (;;) {
        ++cg.waits;
        if ((e = hipMemcpyAsync(bw.h_state, bw.d_state, sizeof(BCGSState), hipMemcpyDeviceToHost, s)) != hipSuccess)
            return cg_hip(e, "KSPSolve_BCGS poll");
        if ((rc = op.wait(s))) return rc;
        if (bw.h_state->done || launched >= cg.max_it) break;
        const int32_t n = std::min<int32_t>(std::max<int32_t>(1, cg.poll), cg.max_it - launched);
        for (int32_t j = 0; j < n; ++j)
            if ((rc = bcgs_iteration(cg, bw, op, x, p, s))) return rc;
        launched += n;
    }
    hipLaunchKernelGGL(kb_final_x, vg, vt, 0, s, m, cg.d_p, x, bw.d_state);
    if ((e = hipGetLastError()) != hipSuccess ||
        (e = hipMemcpyAsync(bw.h_state, bw.d_state, sizeof(BCGSState), hipMemcpyDeviceToHost, s)) != hipSuccess)
        return cg_hip(e, "KSPSolve_BCGS final update");
    if ((rc = op.wait(s))) return rc;
    ++cg.waits;
    const BCGSState &st = *bw.h_state;
    cg.its = st.its;
    cg.reason = st.reason ? st.reason : AIJHIP_KSP_DIVERGED_ITS;
    cg.rnorm = st.dp;
    const int32_t nh = std::min<int32_t>(cg.hist_cap, st.its + 1);
    cg.hist.resize((size_t)std::max(nh, 0));
    if (nh > 0 &&
        (e = hipMemcpy(cg.hist.data(), cg.d_hist, sizeof(double) * (size_t)nh, hipMemcpyDeviceToHost)) != hipSuccess)
        return cg_hip(e, "residual history");
    return AIJHIP_OK;
}
