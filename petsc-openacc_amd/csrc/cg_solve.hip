// cg_solve.hip — device-resident preconditioned CG, written once for the
// single-GPU handle (ksp.hip) and the row-partitioned one (ksp_mpi.hip).
//
// Restates PETSc 3.7.6 KSPSolve_CG [ext] (src/ksp/ksp/impls/cg/cg.c) with
// KSPConvergedDefault [ext]. Per iteration:
//
//   K1  P = Z            (i = 0)      | P = Z + b P        (VecCopy / VecAYPX)
//   K2  W = A P, partials of P.W      (CGOperator::apply: KSP_MatMult + VecXDot,
//                                      fused into the STREAM SpMV epilogue when
//                                      possible; many ranks: the halo exchange
//                                      beside A_d, then A_o's share)
//   K3  scalar step: dpi, indefinite-matrix check, a = beta / dpi
//   K4  X += a P, R -= a W            (2 x VecAXPY), and for Jacobi / none
//       also Z = D^-1 R with the partials of Z.Z, Z.R, R.R fused in
//   [V-cycle PC: Z = CGOperator::pc_apply(R), then the Z.Z, Z.R partials]
//   K5  scalar step: dp, KSPConvergedDefault, beta, indefinite-PC / beta = 0
//                    checks, b = beta / betaold
//
// K3 / K5 sum this device's partials in a fixed order (k_sum_*) and, on one
// rank, take the scalar step in the same kernel; on many ranks the sums are
// all-reduced first (identical on every rank afterwards, so every rank takes
// the same branch) and k_step_* follows. W shares Z's storage as in PETSc.
// All scalars live on the device; kernels return at once once the device
// flag `done` is set, so the host launches iterations in batches and polls.
#include "cg_solve.h"

#include <algorithm>
#include <cstdlib>

int CGOperator::pc_apply(const double *, double *, hipStream_t, const int *, const double **, int *) {
    return cg_fail(AIJHIP_ERR_STATE, "this CG operator has no V-cycle");
}

int CGOperator::run_batch(const CGRun &R, int32_t n, hipStream_t s) {
    for (int32_t j = 0; j < n; ++j)
        if (const int rc = cg_iteration(R, s)) return rc;
    return AIJHIP_OK;
}

void cg_free(CGSolve &cg) {
    hipFree(cg.d_dinv); hipFree(cg.d_tdinv); hipFree(cg.d_r); hipFree(cg.d_z); hipFree(cg.d_p);
    hipFree(cg.d_part); hipFree(cg.d_red); hipFree(cg.d_hist); hipFree(cg.d_state);
    if (cg.h_state) hipHostFree(cg.h_state);
    cg.d_dinv = cg.d_tdinv = cg.d_r = cg.d_z = cg.d_p = cg.d_part = cg.d_red = cg.d_hist = nullptr;
    cg.d_state = cg.h_state = nullptr;
    cg.implicit_z = false;
    cg.pid = nullptr;
}

int cg_set_up(CGSolve &cg, const aijhip_mat &A, bool implicit_z) {
    cg_free(cg);
    const int64_t m = cg.m = A.m;
    cg.fused = aijhip::stream_dot_fusable(A);
    cg.vec_grid = (int)std::max<int64_t>(1, std::min<int64_t>((m + kVecThreads - 1) / kVecThreads,
                                                              (int64_t)A.n_cu * 8));
    cg.n_dparts = cg.fused ? A.plan.n_blocks : cg.vec_grid;
    const int64_t nparts = std::max<int64_t>((int64_t)kNQ * cg.vec_grid, std::max(1, cg.n_dparts));
    cg.hist_cap = cg.max_it + 2;
    const size_t vb = sizeof(double) * (size_t)std::max<int64_t>(m, 1);
    hipError_t e;
    if ((e = hipMalloc(&cg.d_dinv, vb)) != hipSuccess || (e = hipMalloc(&cg.d_r, vb)) != hipSuccess ||
        (e = hipMalloc(&cg.d_z, vb)) != hipSuccess || (e = hipMalloc(&cg.d_p, vb)) != hipSuccess ||
        (e = hipMalloc(&cg.d_part, sizeof(double) * (size_t)nparts)) != hipSuccess ||
        (e = hipMalloc(&cg.d_red, sizeof(double) * 8)) != hipSuccess ||
        (e = hipMalloc(&cg.d_hist, sizeof(double) * (size_t)cg.hist_cap)) != hipSuccess ||
        (e = hipMalloc(&cg.d_state, sizeof(CGState))) != hipSuccess ||
        (e = hipHostMalloc(&cg.h_state, sizeof(CGState), hipHostMallocDefault)) != hipSuccess) {
        cg_free(cg);
        return cg_hip(e, "KSPSetUp allocation");
    }
    if (m > 0)
        hipLaunchKernelGGL(k_diag_inv, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, nullptr, A.m, A.d_ai, A.d_aj,
                           A.d_aa, cg.d_dinv);
    // Jacobi on row templates: D^-1 per template, Z formed where it is read
    if (implicit_z && cg.pc == AIJHIP_PC_JACOBI && m > 0 && A.plan.d_pid && A.plan.d_pval &&
        !std::getenv("AIJHIP_KSP_EXPLICIT_Z")) {
        const int np = A.plan.n_pat;
        if ((e = hipMalloc(&cg.d_tdinv, sizeof(double) * (size_t)np)) != hipSuccess) {
            cg_free(cg);
            return cg_hip(e, "PCSetUp_Jacobi (templates)");
        }
        hipLaunchKernelGGL(k_tmpl_dinv, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, nullptr, np, A.plan.d_ptab,
                           A.plan.d_pval, cg.d_tdinv);
        cg.implicit_z = true;
        cg.pid = A.plan.d_pid;
    }
    if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) {
        cg_free(cg);
        return cg_hip(e, "PCSetUp_Jacobi");
    }
    return AIJHIP_OK;
}

int cg_set_tolerances(CGSolve &cg, bool set_up, double rtol, double abstol, double dtol, int32_t max_it) {
    if (rtol < 0 || abstol < 0 || dtol <= 0 || max_it < 0) return cg_fail(AIJHIP_ERR_ARG, "bad tolerance");
    cg.rtol = rtol; cg.abstol = abstol; cg.dtol = dtol;
    cg.max_it = max_it;
    if (set_up && cg.hist_cap < max_it + 2) {  // regrow the history only (keeps D^-1 and the PC)
        hipFree(cg.d_hist);
        cg.d_hist = nullptr;
        cg.hist_cap = max_it + 2;
        if (hipMalloc(&cg.d_hist, sizeof(double) * (size_t)cg.hist_cap) != hipSuccess)
            return cg_fail(AIJHIP_ERR_ALLOC, "residual history");
    }
    return AIJHIP_OK;
}

int cg_iteration(const CGRun &R, hipStream_t st) {
    CGSolve &cg = R.cg;
    CGOperator &op = R.op;
    const CGParams &p = R.p;
    const int64_t m = cg.m;
    const dim3 vg(cg.vec_grid), vt(kVecThreads), rt(kRedThreads);
    const int nb = cg.vec_grid;
    double *red = op.multi ? cg.d_red : nullptr;
    int rc;
    if (cg.implicit_z)
        hipLaunchKernelGGL((k_aypx<true, true>), vg, vt, 0, st, m, cg.d_z, cg.d_p, R.x, cg.d_state, cg.d_r, cg.pid,
                           cg.d_tdinv);
    else
        hipLaunchKernelGGL(k_aypx<true>, vg, vt, 0, st, m, cg.d_z, cg.d_p, R.x, cg.d_state);
    // W = A P with the p.w partials (W shares Z's storage)
    if ((rc = op.apply(cg.d_p, cg.d_z, st, cg.d_part, cg.d_state))) return rc;
    if (!cg.fused) hipLaunchKernelGGL(k_dot, vg, vt, 0, st, m, cg.d_p, cg.d_z, cg.d_part, cg.d_state);
    hipLaunchKernelGGL(k_sum_dpi, dim3(1), rt, 0, st, cg.d_part, cg.n_dparts, op.opart, op.nob, red, cg.d_state);
    if (op.multi) {
        if ((rc = op.allreduce(red, 1, st))) return rc;
        hipLaunchKernelGGL(k_step_dpi, dim3(1), dim3(64), 0, st, red, cg.d_state);
    }
    if (cg.implicit_z)
        hipLaunchKernelGGL((k_update<true, true>), vg, vt, 0, st, m, cg.d_r, cg.d_z, cg.d_dinv, cg.d_part, cg.d_state,
                           cg.pc, cg.d_p, nullptr, cg.pid, cg.d_tdinv);
    else
        hipLaunchKernelGGL(k_update<true>, vg, vt, 0, st, m, cg.d_r, cg.d_z, cg.d_dinv, cg.d_part, cg.d_state, cg.pc,
                           cg.d_p, nullptr);
    const double *pz = cg.d_part;
    int nbz = nb;
    if (op.vcycle) {
        // z = B r; z.z and z.r come from the finest post-smoothing when it
        // is fused, else from k_dots
        const double *dots = nullptr;
        int nd = 0;
        if ((rc = op.pc_apply(cg.d_r, cg.d_z, st, &cg.d_state->done, &dots, &nd))) return rc;
        if (dots) {
            pz = dots;
            nbz = nd;
        } else {
            hipLaunchKernelGGL(k_dots, vg, vt, 0, st, m, cg.d_z, cg.d_r, cg.d_part, 0, 1, cg.d_state);
        }
    }
    hipLaunchKernelGGL(k_sum_iter, dim3(1), rt, 0, st, pz, nbz, cg.d_part + 2 * nb, nb, red, cg.d_state, cg.d_hist, p);
    if (op.multi) {
        if ((rc = op.allreduce(red, 3, st))) return rc;
        hipLaunchKernelGGL(k_step_iter, dim3(1), dim3(64), 0, st, red, cg.d_state, cg.d_hist, p);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? AIJHIP_OK : cg_hip(e, "KSPSolve iteration");
}

int cg_solve(CGSolve &cg, CGOperator &op, const double *b, double *x, hipStream_t s) {
    const int64_t m = cg.m;
    if (m > 0 && (!b || !x)) return cg_fail(AIJHIP_ERR_ARG, "NULL vector");
    if (b == x) return cg_fail(AIJHIP_ERR_ARG, "b and x alias");
    const CGRun R{cg, op, x, CGParams{cg.rtol, cg.abstol, cg.dtol, cg.max_it, cg.normtype,
                                      cg.guess_nonzero ? 0 : 1, cg.pc}};
    const CGParams &p = R.p;
    const dim3 vg(cg.vec_grid), vt(kVecThreads), rt(kRedThreads);
    double *red = op.multi ? cg.d_red : nullptr;
    hipError_t e = hipSuccess;
    int rc;
    // KSPSolve [ext]: zero initial guess -> x = 0; else r = A x first.
    if (!cg.guess_nonzero) {
        if (m > 0 && (e = hipMemsetAsync(x, 0, sizeof(double) * (size_t)m, s)) != hipSuccess)
            return cg_hip(e, "KSPSolve init");
    } else if ((rc = op.apply(x, cg.d_r, s, nullptr, nullptr))) {
        return rc;
    }
    // r = b (- A x), z = B r, then ||z|| etc. (summed over all ranks)
    hipLaunchKernelGGL(k_init, vg, vt, 0, s, m, b, cg.d_r, cg.d_z, cg.d_dinv, cg.d_part, p);
    if (op.vcycle) {
        // no stop flag yet: the device state is initialised by the first scalar step
        if (cg.guess_nonzero && cg.normtype != AIJHIP_KSP_NORM_UNPRECONDITIONED) {
            // snorm = |B b| for the preconditioned-norm convergence test
            if ((rc = op.pc_apply(b, cg.d_z, s, nullptr, nullptr, nullptr))) return rc;
            hipLaunchKernelGGL(k_dots, vg, vt, 0, s, m, cg.d_z, nullptr, cg.d_part, 3, -1, nullptr);
        }
        if ((rc = op.pc_apply(cg.d_r, cg.d_z, s, nullptr, nullptr, nullptr))) return rc;
        hipLaunchKernelGGL(k_dots, vg, vt, 0, s, m, cg.d_z, cg.d_r, cg.d_part, 0, 1, nullptr);
    }
    hipLaunchKernelGGL(k_sum_init, dim3(1), rt, 0, s, cg.d_part, cg.vec_grid, red, cg.d_state, cg.d_hist, p);
    if (op.multi) {
        if ((rc = op.allreduce(red, 4, s))) return rc;
        hipLaunchKernelGGL(k_step_init, dim3(1), dim3(64), 0, s, red, cg.d_state, cg.d_hist, p);
    }
    if ((e = hipGetLastError()) != hipSuccess) return cg_hip(e, "KSPSolve init");
    // iterations in batches between polls. The kernels run back to back (a
    // kernel trace of the 300^3 CG + GAMG solve: busy 0.996 of its span), and
    // on one GPU a batch replayed as one captured HIP graph measured slower
    // (solve 0.194 vs 0.188 s, CG + Jacobi 0.331 vs 0.325 s per 400
    // iterations: profiles/r04/s1/graph_ab.txt)
    int32_t launched = 0;
    cg.waits = 0;
    for (;;) {
        ++cg.waits;
        if ((e = hipMemcpyAsync(cg.h_state, cg.d_state, sizeof(CGState), hipMemcpyDeviceToHost, s)) != hipSuccess)
            return cg_hip(e, "KSPSolve poll");
        if ((rc = op.wait(s))) return rc;
        if (cg.h_state->done || launched >= cg.max_it) break;
        const int32_t n = std::min<int32_t>(std::max<int32_t>(1, cg.poll), cg.max_it - launched);
        if ((rc = op.run_batch(R, n, s))) return rc;
        launched += n;
    }
    hipLaunchKernelGGL(k_final_x, vg, vt, 0, s, m, cg.d_p, x, cg.d_state);
    if ((e = hipGetLastError()) != hipSuccess ||
        (e = hipMemcpyAsync(cg.h_state, cg.d_state, sizeof(CGState), hipMemcpyDeviceToHost, s)) != hipSuccess)
        return cg_hip(e, "KSPSolve final update");
    if ((rc = op.wait(s))) return rc;
    ++cg.waits;
    const CGState &st = *cg.h_state;
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
