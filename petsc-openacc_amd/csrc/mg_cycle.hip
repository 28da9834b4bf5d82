// mg_cycle.hip — PCApply_MG, one multiplicative V-cycle (mg_cycle.h).
//
// Level smoothers (the same down and up), after KSPSolve_Richardson /
// KSPSolve_Chebyshev with a Jacobi PC [ext]; nothing is contracted to an FMA
// and every sum is added left to right as written:
//   Richardson(k), scale s (default k = 1, s = 1):
//     zero guess:     x = s (D^-1 b)           (s = 1: x = D^-1 b)
//     every other:    x = x + s (D^-1 (b + (-1) A x))
//   Chebyshev(k) with the host's scale and omega_i (mg_set_smoother):
//     zero guess:     p_km1 = 0;  p_k = scale (D^-1 b)
//     nonzero guess:  p_km1 = x;  p_k = x + scale (D^-1 (b + (-1) A x))
//     step i:         p_kp1 = ((1 - omega_i) p_km1 + omega_i p_k)
//                             + (omega_i scale) (D^-1 (b + (-1) A p_k))
//     (from a zero guess step 0 has no p_km1 term); x = p_k after k steps.
// Coarsest level: preonly + Jacobi. On STREAM-planned levels the smoothing
// passes ride in the SpMV (aijhip::launch_mg_resid / _post / _cheby): the
// zero-guess start is a vector pass, the residual rides in the SpMV after it,
// and interpolation writes t = x + P x_c where the post-smoothing launches
// read it. The steps rotate two of the level's vectors — x and w going down
// (the residual takes r), x and r coming up; a Chebyshev step writes p_kp1 over
// p_km1 — from a first buffer chosen by the parity of the step count, so the
// result lands in x (level 0: the caller's vector) without a copy. Unfused
// levels run MatMult into r and an elementwise pass with the same expression
// (Richardson in place, Chebyshev rotating x and w). Across ranks the fused
// launches run over A_d while the halo moves, then A_o's share is added on
// the boundary rows.
//
// Every halo_post is followed by exactly one halo_finish or halo_abort on
// every return path (mpi_internal.h).
//
// mg_vcycle_multi is the same cycle on k columns at once (single GPU, m_l x k
// interleaved level blocks): the same expressions per entry, every product one
// launch_spmm over all columns with the step in its epilogue (mg_cycle.h).
#include "mg_cycle.h"

#include <algorithm>
#include <cmath>
#include <string>

#include "mpi_internal.h"

namespace {

using aijhip::MGLevelView;
using aijhip_mpi::halo_abort;
using aijhip_mpi::halo_finish;
using aijhip_mpi::halo_post;

// The vector passes. Elementwise, so the grid does not change a bit. SC: the
// factor f (Richardson's scale, Chebyshev's scale) in place of the literal 1.
template <bool SC>
__global__ __launch_bounds__(kVecThreads) void k_jacobi(int64_t n, const double *__restrict__ dinv,
                                                        const double *__restrict__ b, double *x, double f,
                                                        const int *stop) {
    if (stop && *stop) return;
    GRID_STRIDE(i, n) x[i] = SC ? f * (dinv[i] * b[i]) : dinv[i] * b[i];
}

// The same on row templates: D^-1 of row i is tdinv[pid[i]] (the same bits)
template <bool SC>
__global__ __launch_bounds__(kVecThreads) void k_jacobi_t(int64_t n, const uint8_t *__restrict__ pid,
                                                          const double *__restrict__ tdinv,
                                                          const double *__restrict__ b, double *x, double f,
                                                          const int *stop) {
    if (stop && *stop) return;
    GRID_STRIDE(i, n) x[i] = SC ? f * (tdinv[pid[i]] * b[i]) : tdinv[pid[i]] * b[i];
}

// MatResidual: r = b + (-1) r, where r holds A x on entry (VecAYPX(r,-1,b)).
__global__ __launch_bounds__(kVecThreads) void k_resid(int64_t n, const double *__restrict__ b, double *r,
                                                       const int *stop) {
    if (stop && *stop) return;
    GRID_STRIDE(i, n) r[i] = b[i] + (-1.0) * r[i];
}

// y = x + f (D^-1 (b - A x)) with ax = A x; y may be x
template <bool SC>
__global__ __launch_bounds__(kVecThreads) void k_richardson(int64_t n, const double *__restrict__ dinv,
                                                            const double *__restrict__ b,
                                                            const double *__restrict__ ax, const double *x, double *y,
                                                            double f, const int *stop) {
    if (stop && *stop) return;
    GRID_STRIDE(i, n) y[i] = x[i] + (SC ? f : 1.0) * (dinv[i] * (b[i] + (-1.0) * ax[i]));
}

// One Chebyshev step with ax = A p_k (OpMgCheby's expression); out may be pm1
template <bool P0>
__global__ __launch_bounds__(kVecThreads) void k_cheby_step(int64_t n, const double *__restrict__ dinv,
                                                            const double *__restrict__ b,
                                                            const double *__restrict__ ax, const double *pm1,
                                                            const double *__restrict__ pk, double *out, double c0,
                                                            double c1, double c2, const int *stop) {
    if (stop && *stop) return;
    GRID_STRIDE(i, n) {
        const double corr = c2 * (dinv[i] * (b[i] + (-1.0) * ax[i]));
        out[i] = P0 ? c1 * pk[i] + corr : (c0 * pm1[i] + c1 * pk[i]) + corr;
    }
}

// y[o] = y[o] + (f scale[o]) * (-(A_o g)_o) over A_o's rows (scale NULL: 1):
// the off-diagonal block's share of a fused residual (r = b - A_d x - A_o g)
// or smoothing step (x = t + f D^-1 (b - A_d t - A_o g)) on the boundary rows
__global__ __launch_bounds__(256) void k_offdiag_axpy(int32_t nr, const int32_t *__restrict__ rai,
                                                      const int32_t *__restrict__ ridx, const int32_t *__restrict__ aj,
                                                      const double *__restrict__ aa, const double *__restrict__ g,
                                                      const double *__restrict__ scale, double f, double *y,
                                                      const int *stop) {
    if (stop && *stop) return;
    for (int32_t q = blockIdx.x * 256 + threadIdx.x; q < nr; q += gridDim.x * 256) {
        const int32_t o = ridx ? ridx[q] : q;
        double sum = 0.0;
        for (int32_t k = rai[q]; k < rai[q + 1]; ++k) sum += aa[k] * g[aj[k]];
        y[o] = y[o] + (scale ? f * scale[o] : 1.0) * (-sum);
    }
}

// The multi-column V-cycle's vector pass over an m x k interleaved level block
// (leading dimension k): x = f (D^-1 b) with dinv[i / k] — the zero-guess
// start of either smoother and the coarse solve (f = 1.0 multiplies to the bits
// of k_jacobi's literal form). V2 (k even): n counts pairs, 16-byte accesses.
template <bool V2>
__global__ __launch_bounds__(kVecThreads) void k_jacobi_multi(int64_t n, int32_t k, const double *__restrict__ dinv,
                                                              const double *__restrict__ b, double *x, double f,
                                                              const int *stop) {
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    if (stop && *stop) return;
    GRID_STRIDE(i, n) {
        if constexpr (V2) {
            const double di = dinv[2 * i / k];
            const f64x2 bv = reinterpret_cast<const f64x2 *>(b)[i];
            f64x2 xv;
            xv.x = f * (di * bv.x);
            xv.y = f * (di * bv.y);
            reinterpret_cast<f64x2 *>(x)[i] = xv;
        } else {
            x[i] = f * (dinv[i / k] * b[i]);
        }
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
int offdiag_axpy(const MGLevelView &L, const double *scale, double f, double *y, hipStream_t s, const int *stop) {
    if (!L.Ao) return AIJHIP_OK;
    const aijhip::RowList R = aijhip::row_list(*L.Ao);
    if (R.nr == 0) return AIJHIP_OK;
    hipLaunchKernelGGL(k_offdiag_axpy, dim3((unsigned)((R.nr + 255) / 256)), dim3(256), 0, s, R.nr, R.rai, R.ridx,
                       L.Ao->d_aj, L.Ao->d_aa, L.op->d_ghost, scale, f, y, stop);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? AIJHIP_OK : gerr(e, "off-diagonal smoothing share");
}

int sfail(const char *msg) {
    aijhip::set_error(std::string("MG smoother: ") + msg);
    return AIJHIP_ERR_ARG;
}

}  // namespace

extern "C" {

int aijhip_mg_smoother_default(aijhip_mg_smoother_t *s) {
    if (!s) return sfail("NULL argument");
    s->type = AIJHIP_MG_SMOOTH_RICHARDSON;
    s->its = 1;
    s->richardson_scale = 1.0;
    s->cheby_lo = 0.05;
    s->cheby_hi = 1.05;
    return AIJHIP_OK;
}

int aijhip_mg_cheby_coefficients(double emax, double emin, int32_t k, double *scale, double *omega) {
    if (!scale || !omega) return sfail("NULL argument");
    if (k < 1 || k > AIJHIP_MG_MAX_ITS) return sfail("its must be in 1..16");
    if (!(emin > 0.0) || !(emax > emin)) return sfail("Chebyshev needs 0 < emin < emax");
    *scale = 2.0 / (emax + emin);
    const double alpha = 1.0 - *scale * emin;
    const double mu = 1.0 / alpha, omegaprod = 2.0 / alpha;
    double c_km1 = 1.0, c_k = mu;
    for (int32_t i = 0; i < k; ++i) {
        const double c_kp1 = 2.0 * mu * c_k - c_km1;
        omega[i] = omegaprod * c_k / c_kp1;
        c_km1 = c_k;
        c_k = c_kp1;
    }
    return AIJHIP_OK;
}

}  // extern "C"

namespace aijhip {

int mg_check_smoother(const aijhip_mg_smoother_t &s, const aijhip_gamg_params_t *p) {
    if (s.type != AIJHIP_MG_SMOOTH_RICHARDSON && s.type != AIJHIP_MG_SMOOTH_CHEBYSHEV)
        return sfail("unknown type (richardson or chebyshev)");
    if (s.its < 1 || s.its > AIJHIP_MG_MAX_ITS) return sfail("its must be in 1..16");
    if (!(s.cheby_lo > 0.0)) return sfail("Chebyshev bounds: lo must be positive");
    if (!(s.cheby_lo < s.cheby_hi)) return sfail("Chebyshev bounds: lo must be below hi");
    if (!std::isfinite(s.richardson_scale) || !std::isfinite(s.cheby_hi))
        return sfail("the Richardson scale and the Chebyshev bounds must be finite");
    if (p && s.type == AIJHIP_MG_SMOOTH_CHEBYSHEV && p->nsmooths <= 0)
        return sfail("Chebyshev needs each level's emax(D^-1 A) estimate, which the set-up makes only to smooth the "
                     "prolongator: nsmooths = 0 leaves none");
    return AIJHIP_OK;
}

int mg_set_smoother(const aijhip_mg_smoother_t &s, double lambda, MGLevelView &L) {
    const int rc = mg_check_smoother(s);
    if (rc) return rc;
    L.smooth = s.type;
    L.its = s.its;
    L.rscale = s.richardson_scale;
    L.cmin = L.cmax = L.scale = 0.0;
    if (s.type != AIJHIP_MG_SMOOTH_CHEBYSHEV) return AIJHIP_OK;
    if (!(lambda > 0.0)) return sfail("Chebyshev: the level has no emax(D^-1 A) estimate");
    L.cmin = s.cheby_lo * lambda;
    L.cmax = s.cheby_hi * lambda;
    return aijhip_mg_cheby_coefficients(L.cmax, L.cmin, L.its, &L.scale, L.omega);
}

bool mg_smoother_needs_w(const MGLevelView &L) {
    return L.smooth == AIJHIP_MG_SMOOTH_CHEBYSHEV || (L.fused && L.its > 1);
}

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
    // x = f (D^-1 b): the zero-guess start of either smoother, the coarse solve (f = 1)
    auto jacobi = [&](const MGLevelView &L, int l, double f, double *x) {
        const dim3 g = grid(L);
        const int64_t m = L.m;
        if (L.fused && L.tdinv && l < nl - 1) {
            const uint8_t *pid = L.Ad->plan.d_pid;
            if (f == 1.0) hipLaunchKernelGGL(k_jacobi_t<false>, g, t, 0, s, m, pid, L.tdinv, B(l), x, f, stop);
            else hipLaunchKernelGGL(k_jacobi_t<true>, g, t, 0, s, m, pid, L.tdinv, B(l), x, f, stop);
        } else if (f == 1.0) {
            hipLaunchKernelGGL(k_jacobi<false>, g, t, 0, s, m, L.dinv, B(l), x, f, stop);
        } else {
            hipLaunchKernelGGL(k_jacobi<true>, g, t, 0, s, m, L.dinv, B(l), x, f, stop);
        }
    };
    // One smoothing step from pk with one product of A. cheby: out = (c0 pm1
    // + c1 pk) + c2 D^-1 (b - A pk) (pm1 NULL: no c0 term), out may be pm1;
    // else Richardson: out = pk + c2 D^-1 (b - A pk). Fused: out != pk, the
    // launch over A_d while the halo moves and A_o's share after; unfused:
    // MatMult into r, then the elementwise pass. dp: CG's z.z / z.b partials.
    auto step = [&](const MGLevelView &L, int l, bool cheby, const double *pm1, const double *pk, double *out,
                    double c0, double c1, double c2, double *dp) -> int {
        if (!L.fused) {
            int rc1 = mult(L, pk, L.r, s, stop);
            if (rc1) return rc1;
            const dim3 g = grid(L);
            const int64_t m = L.m;
            if (!cheby && c2 == 1.0)
                hipLaunchKernelGGL(k_richardson<false>, g, t, 0, s, m, L.dinv, B(l), L.r, pk, out, c2, stop);
            else if (!cheby)
                hipLaunchKernelGGL(k_richardson<true>, g, t, 0, s, m, L.dinv, B(l), L.r, pk, out, c2, stop);
            else if (!pm1)
                hipLaunchKernelGGL(k_cheby_step<true>, g, t, 0, s, m, L.dinv, B(l), L.r, pm1, pk, out, c0, c1, c2,
                                   stop);
            else
                hipLaunchKernelGGL(k_cheby_step<false>, g, t, 0, s, m, L.dinv, B(l), L.r, pm1, pk, out, c0, c1, c2,
                                   stop);
            return AIJHIP_OK;
        }
        const bool ex = exchanges(L.op);
        int rc1;
        if (ex && (rc1 = halo_post(L.op, pk, s))) return rc1;
        const hipError_t e1 =
            cheby ? launch_mg_cheby(*L.Ad, pm1, pk, B(l), L.dinv, out, c0, c1, c2, dp, s, stop, L.tdinv)
                  : launch_mg_post(*L.Ad, pk, B(l), L.dinv, out, dp, s, stop, L.tdinv, c2);
        if (e1 != hipSuccess) return ex ? halo_abort(L.op, s, gerr(e1, "smoothing")) : gerr(e1, "smoothing");
        if (ex && (rc1 = halo_finish(L.op, s))) return rc1;
        return offdiag_axpy(L, L.dinv, c2, out, s, stop);
    };
    for (int l = 0; l < nl; ++l) {
        const MGLevelView &L = lv[l];
        if (l == nl - 1) {  // coarse: preonly + Jacobi, x = D^-1 b
            jacobi(L, l, 1.0, X(l));
            break;
        }
        // smoothd from a zero guess: the start, then n steps rotating two
        // buffers (unfused Richardson: in place) so that the last lands in x
        const bool cheby = L.smooth == AIJHIP_MG_SMOOTH_CHEBYSHEV;
        const int n = cheby ? L.its : L.its - 1;
        const bool inplace = !cheby && !L.fused;
        if (n > 0 && !inplace && !L.w) return gerr(hipErrorInvalidValue, "no smoother work vector");
        double *cur = inplace || n % 2 == 0 ? X(l) : L.w, *oth = inplace ? X(l) : n % 2 == 0 ? L.w : X(l);
        jacobi(L, l, cheby ? L.scale : L.rscale, cur);
        for (int i = 0; i < n; ++i) {
            if (cheby)
                rc = step(L, l, true, i == 0 ? nullptr : oth, cur, oth, 1.0 - L.omega[i], L.omega[i],
                          L.omega[i] * L.scale, nullptr);
            else
                rc = step(L, l, false, nullptr, cur, oth, 0.0, 0.0, L.rscale, nullptr);
            if (rc) return rc;
            std::swap(cur, oth);
        }
        const dim3 g = grid(L);
        if (L.fused) {  // r = b - A x in the SpMV epilogue (over A_d while the halo moves)
            const bool ex = exchanges(L.op);
            if (ex && (rc = halo_post(L.op, X(l), s))) return rc;
            if ((e = launch_mg_resid(*L.Ad, X(l), B(l), L.r, s, stop)) != hipSuccess)
                return ex ? halo_abort(L.op, s, gerr(e, "residual")) : gerr(e, "residual");
            if (ex && (rc = halo_finish(L.op, s))) return rc;
            if ((rc = offdiag_axpy(L, nullptr, 1.0, L.r, s, stop))) return rc;
        } else {  // MatMult, then the residual
            if ((rc = mult(L, X(l), L.r, s, stop))) return rc;
            hipLaunchKernelGGL(k_resid, g, t, 0, s, (int64_t)L.m, B(l), L.r, stop);
        }
        // MatRestrict: b_{l+1} = P^T r
        if ((rc = restrict_to(L, L.r, lv[l + 1].b, s, stop))) return rc;
    }
    for (int l = nl - 2; l >= 0; --l) {
        const MGLevelView &L = lv[l];
        // MatInterpolateAdd t = x + P x_c, then smoothu from t: n steps (the
        // Chebyshev start x + scale D^-1 (b - A x) is a Richardson step).
        // Fused: t goes to the scratch r or stays in x, by n's parity, the
        // steps rotate x and r; unfused: r takes the products, Richardson runs
        // in place (PETSc's order) and Chebyshev rotates x and w.
        const bool cheby = L.smooth == AIJHIP_MG_SMOOTH_CHEBYSHEV;
        const int n = cheby ? L.its + 1 : L.its;
        const bool inplace = !cheby && !L.fused;
        double *alt = L.fused ? L.r : L.w;
        if (!inplace && !alt) return gerr(hipErrorInvalidValue, "no smoother work vector");
        double *cur = inplace || n % 2 == 0 ? X(l) : alt, *oth = inplace ? X(l) : n % 2 == 0 ? alt : X(l);
        if ((rc = transfer(L, X(l + 1), X(l), cur, s, stop))) return rc;
        double *dp = (l == 0 && L.fused && dots && !L.Ao) ? dots : nullptr;
        for (int i = 0; i < n; ++i) {
            double *dpi = i == n - 1 ? dp : nullptr;
            if (!cheby) {
                rc = step(L, l, false, nullptr, cur, oth, 0.0, 0.0, L.rscale, dpi);
            } else if (i == 0) {
                rc = step(L, l, false, nullptr, cur, oth, 0.0, 0.0, L.scale, dpi);
            } else {  // p_kp1 over p_km1 (cur holds p_k, oth p_km1)
                const double om = L.omega[i - 1];
                rc = step(L, l, true, oth, cur, oth, 1.0 - om, om, om * L.scale, dpi);
            }
            if (rc) return rc;
            std::swap(cur, oth);
        }
        if (dp && dots_done) *dots_done = true;
    }
    e = hipGetLastError();
    return e == hipSuccess ? AIJHIP_OK : gerr(e, "kernel launch");
}

void mg_multi_free(MGMultiBlocks &mb) {
    for (MGMultiBlocks::Level &L : mb.lev) {
        hipFree(L.b); hipFree(L.x); hipFree(L.r); hipFree(L.w);
    }
    mb.lev.clear();
    mb.cap_k = 0;
}

int mg_multi_reserve(const std::vector<MGLevelView> &lv, int32_t kmax, MGMultiBlocks &mb) {
    if (kmax <= mb.cap_k && mb.lev.size() == lv.size()) return AIJHIP_OK;
    mg_multi_free(mb);
    mb.lev.assign(lv.size(), MGMultiBlocks::Level());
    for (size_t l = 0; l < lv.size(); ++l) {
        const size_t vb = sizeof(double) * (size_t)std::max<int32_t>(lv[l].m, 1) * (size_t)kmax;
        MGMultiBlocks::Level &L = mb.lev[l];
        hipError_t e;
        if ((e = hipMalloc(&L.b, vb)) != hipSuccess || (e = hipMalloc(&L.x, vb)) != hipSuccess ||
            (e = hipMalloc(&L.r, vb)) != hipSuccess || (e = hipMalloc(&L.w, vb)) != hipSuccess) {
            mg_multi_free(mb);
            return gerr(e, "multi-column level blocks");
        }
    }
    mb.cap_k = kmax;
    return AIJHIP_OK;
}

int mg_vcycle_multi(const std::vector<MGLevelView> &lv, const MGMultiBlocks &mb, int32_t k, const double *B0,
                    double *X0, hipStream_t s, const int *stop) {
    const int nl = (int)lv.size();
    if (k < 1 || k > mb.cap_k || (int)mb.lev.size() != nl || nl < 1)
        return gerr(hipErrorInvalidValue, "multi-column level blocks not reserved for this width");
    for (const MGLevelView &L : lv)
        if (L.op || L.Ao || L.Po) return gerr(hipErrorInvalidValue, "the multi-column V-cycle is single-GPU");
    const int64_t ld = k;
    const int il = AIJHIP_DENSE_INTERLEAVED;
    auto B = [&](int l) { return l == 0 ? B0 : (const double *)mb.lev[l].b; };
    auto X = [&](int l) { return l == 0 ? X0 : mb.lev[l].x; };
    // x = f (D^-1 b) over the level's m_l k entries
    auto jacobi = [&](const MGLevelView &L, int l, double f, double *x) {
        // pairs only where every 16-byte access is aligned (level 0's blocks are the caller's)
        const bool v2 = (k & 1) == 0 &&
                        ((reinterpret_cast<uintptr_t>(B(l)) | reinterpret_cast<uintptr_t>(x)) & 15) == 0;
        const int64_t n = (int64_t)L.m * k / (v2 ? 2 : 1);
        const dim3 g((unsigned)std::max<int64_t>(
            1, std::min<int64_t>((n + kVecThreads - 1) / kVecThreads, (int64_t)L.Ad->n_cu * 8)));
        if (v2) hipLaunchKernelGGL(k_jacobi_multi<true>, g, dim3(kVecThreads), 0, s, n, k, L.dinv, B(l), x, f, stop);
        else hipLaunchKernelGGL(k_jacobi_multi<false>, g, dim3(kVecThreads), 0, s, n, k, L.dinv, B(l), x, f, stop);
    };
    // One smoothing step from pk, one product of A_l with its epilogue:
    // Richardson out = pk + c2 D^-1 (b - A pk), or Chebyshev out = (c0 pm1 +
    // c1 pk) + c2 D^-1 (b - A pk) (pm1 NULL: no c0 term). out != pk.
    auto step = [&](const MGLevelView &L, int l, bool cheby, const double *pm1, const double *pk, double *out,
                    double c0, double c1, double c2) -> int {
        SpmmOp op;
        op.op = cheby ? kSpmmCheby : kSpmmPost;
        op.B = B(l);
        op.PM1 = pm1;
        op.dinv = L.dinv;
        op.c0 = c0; op.c1 = c1; op.c2 = c2;
        const hipError_t e1 = launch_spmm(*L.Ad, k, il, pk, ld, out, ld, s, op, stop);
        return e1 == hipSuccess ? AIJHIP_OK : gerr(e1, "multi-column smoothing");
    };
    int rc;
    hipError_t e;
    for (int l = 0; l < nl; ++l) {
        const MGLevelView &L = lv[l];
        if (l == nl - 1) {  // coarse: preonly + Jacobi
            jacobi(L, l, 1.0, X(l));
            break;
        }
        // smoothd from a zero guess, rotating x and w so that the last step lands in x
        const bool cheby = L.smooth == AIJHIP_MG_SMOOTH_CHEBYSHEV;
        const int n = cheby ? L.its : L.its - 1;
        double *w = mb.lev[l].w, *r = mb.lev[l].r;
        double *cur = n % 2 == 0 ? X(l) : w, *oth = n % 2 == 0 ? w : X(l);
        jacobi(L, l, cheby ? L.scale : L.rscale, cur);
        for (int i = 0; i < n; ++i) {
            if (cheby)
                rc = step(L, l, true, i == 0 ? nullptr : oth, cur, oth, 1.0 - L.omega[i], L.omega[i],
                          L.omega[i] * L.scale);
            else
                rc = step(L, l, false, nullptr, cur, oth, 0.0, 0.0, L.rscale);
            if (rc) return rc;
            std::swap(cur, oth);
        }
        SpmmOp res;  // r = b - A x
        res.op = kSpmmResid;
        res.B = B(l);
        if ((e = launch_spmm(*L.Ad, k, il, X(l), ld, r, ld, s, res, stop)) != hipSuccess)
            return gerr(e, "multi-column residual");
        // MatRestrict: b_{l+1} = P^T r
        if ((e = launch_spmm(*L.Pd->transpose, k, il, r, ld, mb.lev[l + 1].b, ld, s, SpmmOp(), stop)) != hipSuccess)
            return gerr(e, "multi-column restriction");
    }
    for (int l = nl - 2; l >= 0; --l) {
        const MGLevelView &L = lv[l];
        // MatInterpolateAdd t = x + P x_c into x or r by the step count's
        // parity, then smoothu from t rotating x and r (mg_vcycle's fused form)
        const bool cheby = L.smooth == AIJHIP_MG_SMOOTH_CHEBYSHEV;
        const int n = cheby ? L.its + 1 : L.its;
        double *alt = mb.lev[l].r;
        double *cur = n % 2 == 0 ? X(l) : alt, *oth = n % 2 == 0 ? alt : X(l);
        SpmmOp add;
        add.op = kSpmmAdd;
        add.B = X(l);
        if ((e = launch_spmm(*L.Pd, k, il, X(l + 1), ld, cur, ld, s, add, stop)) != hipSuccess)
            return gerr(e, "multi-column interpolation");
        for (int i = 0; i < n; ++i) {
            if (!cheby) {
                rc = step(L, l, false, nullptr, cur, oth, 0.0, 0.0, L.rscale);
            } else if (i == 0) {
                rc = step(L, l, false, nullptr, cur, oth, 0.0, 0.0, L.scale);
            } else {  // p_kp1 over p_km1 (cur holds p_k, oth p_km1)
                const double om = L.omega[i - 1];
                rc = step(L, l, true, oth, cur, oth, 1.0 - om, om, om * L.scale);
            }
            if (rc) return rc;
            std::swap(cur, oth);
        }
    }
    e = hipGetLastError();
    return e == hipSuccess ? AIJHIP_OK : gerr(e, "kernel launch");
}

}  // namespace aijhip
