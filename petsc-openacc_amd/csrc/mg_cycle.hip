// mg_cycle.hip — PCApply_MG, one multiplicative V-cycle (mg_cycle.h).
//
// Smoother: KSPSolve_Richardson with one iteration, scale 1, Jacobi PC [ext]:
//   zero guess:     x = 0 + 1.0 * (D^-1 b)           = D^-1 b
//   nonzero guess:  x = x + 1.0 * (D^-1 (b + (-1) A x))
// Coarsest level: preonly + Jacobi. On STREAM-planned levels the smoothing
// passes ride in the SpMV (aijhip::launch_mg_resid / _post): the residual
// rides in the SpMV after the x = D^-1 b vector pass, and interpolation
// writes t = x + P x_c to the level's scratch so the post-smoothing launch
// reads t and writes x. Across ranks those launches run over A_d while the
// halo moves, then A_o's share is added on the boundary rows.
//
// Every halo_post is followed by exactly one halo_finish or halo_abort on
// every return path (mpi_internal.h).
#include "mg_cycle.h"

#include <algorithm>
#include <string>

#include "mpi_internal.h"

namespace {

using aijhip::MGLevelView;
using aijhip_mpi::halo_abort;
using aijhip_mpi::halo_finish;
using aijhip_mpi::halo_post;

// The vector passes. Elementwise, so the grid does not change a bit.
__global__ __launch_bounds__(kVecThreads) void k_jacobi(int64_t n, const double *__restrict__ dinv,
                                                        const double *__restrict__ b, double *x,
                                                        const int *stop) {
    if (stop && *stop) return;
    GRID_STRIDE(i, n) x[i] = dinv[i] * b[i];
}

// The same on row templates: D^-1 of row i is tdinv[pid[i]] (the same bits)
__global__ __launch_bounds__(kVecThreads) void k_jacobi_t(int64_t n, const uint8_t *__restrict__ pid,
                                                          const double *__restrict__ tdinv,
                                                          const double *__restrict__ b, double *x, const int *stop) {
    if (stop && *stop) return;
    GRID_STRIDE(i, n) x[i] = tdinv[pid[i]] * b[i];
}

// MatResidual: r = b + (-1) r, where r holds A x on entry (VecAYPX(r,-1,b)).
__global__ __launch_bounds__(kVecThreads) void k_resid(int64_t n, const double *__restrict__ b, double *r,
                                                       const int *stop) {
    if (stop && *stop) return;
    GRID_STRIDE(i, n) r[i] = b[i] + (-1.0) * r[i];
}

__global__ __launch_bounds__(kVecThreads) void k_richardson(int64_t n, const double *__restrict__ dinv,
                                                            const double *__restrict__ b,
                                                            const double *__restrict__ ax, double *x,
                                                            const int *stop) {
    if (stop && *stop) return;
    GRID_STRIDE(i, n) x[i] = x[i] + 1.0 * (dinv[i] * (b[i] + (-1.0) * ax[i]));
}

// y[o] = y[o] + scale[o] * (-(A_o g)_o) over A_o's rows (scale NULL: 1): the
// off-diagonal block's share of a fused residual (r = b - A_d x - A_o g) or
// post-smoothing (x = t + D^-1 (b - A_d t - A_o g)) on the boundary rows
__global__ __launch_bounds__(256) void k_offdiag_axpy(int32_t nr, const int32_t *__restrict__ rai,
                                                      const int32_t *__restrict__ ridx, const int32_t *__restrict__ aj,
                                                      const double *__restrict__ aa, const double *__restrict__ g,
                                                      const double *__restrict__ scale, double *y, const int *stop) {
    if (stop && *stop) return;
    for (int32_t q = blockIdx.x * 256 + threadIdx.x; q < nr; q += gridDim.x * 256) {
        const int32_t o = ridx ? ridx[q] : q;
        double sum = 0.0;
        for (int32_t k = rai[q]; k < rai[q + 1]; ++k) sum += aa[k] * g[aj[k]];
        y[o] = y[o] + (scale ? scale[o] : 1.0) * (-sum);
    }
}

int gerr(hipError_t e, const char *what) {
    aijhip::set_error(std::string("GAMG V-cycle: ") + what + ": " + hipGetErrorString(e));
    return AIJHIP_ERR_HIP;
}

bool exchanges(const aijhip_mpiaij *M) { return M && (M->n_send > 0 || M->n_ghost > 0); }

// y = A x: MatMult_MPIAIJ through the level's halo, or the plain product
int mult(const MGLevelView &L, const double *x, double *y, hipStream_t s, const int *stop) {
    if (L.op) return aijhip_mpi::mpiaij_apply(L.op, x, y, s, nullptr, nullptr, nullptr, false, stop);
    const hipError_t e = aijhip::launch_mult(*L.Ad, x, nullptr, y, false, s, stop);
    return e == hipSuccess ? AIJHIP_OK : gerr(e, "product");
}

// y = P x_c (+ z) through the halo of the coarse level: the exchange of x_c
// overlaps P_d x_c
int transfer(const MGLevelView &L, const double *xc, const double *z, double *y, hipStream_t s, const int *stop) {
    aijhip_mpiaij *halo_op = L.op_next;
    const bool exch = exchanges(halo_op);
    int rc = exch ? halo_post(halo_op, xc, s) : AIJHIP_OK;
    if (rc) return rc;
    hipError_t e = aijhip::launch_mult(*L.Pd, xc, z, y, true, s, stop);
    if (e != hipSuccess)
        return exch ? halo_abort(halo_op, s, gerr(e, "transfer product")) : gerr(e, "transfer product");
    if (exch && (rc = halo_finish(halo_op, s))) return rc;
    if (L.Po && (e = aijhip::launch_mult(*L.Po, halo_op->d_ghost, y, y, true, s, stop)) != hipSuccess)
        return gerr(e, "transfer ghost product");
    return AIJHIP_OK;
}

// MatRestrict as MatMultTranspose_MPIAIJ: b = P_d^T r, then P_o^T r (one
// value per ghost coarse slot of level l+1, in that level's ghost vector)
// sent back to the slots' owners and added (halo_reverse_add). An aggregate
// may have members on other ranks up to two steps from its root (PETSc's
// parallel MIS), and P's smoothing reaches one more, so the fine rows with
// entries in a rank's coarse columns are not all ghosts of its level-l halo:
// the sums travel with the coarse level's plan instead.
int restrict_to(const MGLevelView &L, const double *r, double *b, hipStream_t s, const int *stop) {
    hipError_t e = aijhip::launch_mult(*L.Pd->transpose, r, nullptr, b, false, s, stop);
    if (e != hipSuccess) return gerr(e, "restriction");
    aijhip_mpiaij *M = L.op_next;
    if (!exchanges(M)) return AIJHIP_OK;
    double *t = M->d_ghost;
    if (L.Po && L.Po->transpose) e = aijhip::launch_mult(*L.Po->transpose, r, nullptr, t, false, s, stop);
    else if (M->n_ghost > 0) e = hipMemsetAsync(t, 0, sizeof(double) * (size_t)M->n_ghost, s);
    if (e != hipSuccess) return gerr(e, "restriction (off-rank share)");
    return aijhip_mpi::halo_reverse_add(M, t, b, s);
}

// The A_o correction of a fused smoothing launch (after the halo landed).
int offdiag_axpy(const MGLevelView &L, const double *scale, double *y, hipStream_t s, const int *stop) {
    if (!L.Ao) return AIJHIP_OK;
    const aijhip::RowList R = aijhip::row_list(*L.Ao);
    if (R.nr == 0) return AIJHIP_OK;
    hipLaunchKernelGGL(k_offdiag_axpy, dim3((unsigned)((R.nr + 255) / 256)), dim3(256), 0, s, R.nr, R.rai, R.ridx,
                       L.Ao->d_aj, L.Ao->d_aa, L.op->d_ghost, scale, y, stop);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? AIJHIP_OK : gerr(e, "off-diagonal smoothing share");
}

}  // namespace

namespace aijhip {

int mg_vcycle(const std::vector<MGLevelView> &lv, const double *b0, double *x0, hipStream_t s, const int *stop,
              double *dots, bool *dots_done) {
    const int nl = (int)lv.size();
    if (dots_done) *dots_done = false;
    auto B = [&](int l) { return l == 0 ? b0 : (const double *)lv[l].b; };
    auto X = [&](int l) { return l == 0 ? x0 : lv[l].x; };
    auto grid = [](const MGLevelView &L) {
        return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(((int64_t)L.m + kVecThreads - 1) / kVecThreads,
                                                                     (int64_t)L.Ad->n_cu * 8)));
    };
    const dim3 t(kVecThreads);
    int rc;
    hipError_t e;
    for (int l = 0; l < nl; ++l) {
        const MGLevelView &L = lv[l];
        const dim3 g = grid(L);
        // smoothd (coarse: preonly + Jacobi): x = D^-1 b
        if (L.fused && L.tdinv && l < nl - 1)
            hipLaunchKernelGGL(k_jacobi_t, g, t, 0, s, (int64_t)L.m, L.Ad->plan.d_pid, L.tdinv, B(l), X(l), stop);
        else
            hipLaunchKernelGGL(k_jacobi, g, t, 0, s, (int64_t)L.m, L.dinv, B(l), X(l), stop);
        if (l == nl - 1) break;
        if (L.fused) {  // r = b - A x in the SpMV epilogue (over A_d while the halo moves)
            const bool ex = exchanges(L.op);
            if (ex && (rc = halo_post(L.op, X(l), s))) return rc;
            if ((e = launch_mg_resid(*L.Ad, X(l), B(l), L.r, s, stop)) != hipSuccess)
                return ex ? halo_abort(L.op, s, gerr(e, "residual")) : gerr(e, "residual");
            if (ex && (rc = halo_finish(L.op, s))) return rc;
            if ((rc = offdiag_axpy(L, nullptr, L.r, s, stop))) return rc;
        } else {  // MatMult, then the residual
            if ((rc = mult(L, X(l), L.r, s, stop))) return rc;
            hipLaunchKernelGGL(k_resid, g, t, 0, s, (int64_t)L.m, B(l), L.r, stop);
        }
        // MatRestrict: b_{l+1} = P^T r
        if ((rc = restrict_to(L, L.r, lv[l + 1].b, s, stop))) return rc;
    }
    for (int l = nl - 2; l >= 0; --l) {
        const MGLevelView &L = lv[l];
        if (L.fused) {
            // MatInterpolateAdd into the scratch: t = x + P x_c, then smoothu
            // x = t + D^-1 (b - A t) in the SpMV epilogue
            if ((rc = transfer(L, X(l + 1), X(l), L.r, s, stop))) return rc;
            double *dp = (l == 0 && dots && !L.Ao) ? dots : nullptr;
            const bool ex = exchanges(L.op);
            if (ex && (rc = halo_post(L.op, L.r, s))) return rc;
            if ((e = launch_mg_post(*L.Ad, L.r, B(l), L.dinv, X(l), dp, s, stop, L.tdinv)) != hipSuccess)
                return ex ? halo_abort(L.op, s, gerr(e, "post-smoothing")) : gerr(e, "post-smoothing");
            if (ex && (rc = halo_finish(L.op, s))) return rc;
            if ((rc = offdiag_axpy(L, L.dinv, X(l), s, stop))) return rc;
            if (dp && dots_done) *dots_done = true;
        } else {
            // MatInterpolateAdd: x = x + P x_c; smoothu: x = x + D^-1 (b - A x)
            if ((rc = transfer(L, X(l + 1), X(l), X(l), s, stop))) return rc;
            if ((rc = mult(L, X(l), L.r, s, stop))) return rc;
            hipLaunchKernelGGL(k_richardson, grid(L), t, 0, s, (int64_t)L.m, L.dinv, B(l), L.r, X(l), stop);
        }
    }
    e = hipGetLastError();
    return e == hipSuccess ? AIJHIP_OK : gerr(e, "kernel launch");
}

}  // namespace aijhip
