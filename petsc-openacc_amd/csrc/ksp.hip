// ksp.hip — device-resident preconditioned CG (include/aijhip_ksp.h).
//
// Restates PETSc 3.7.6 KSPSolve_CG [ext] (src/ksp/ksp/impls/cg/cg.c) with
// KSPConvergedDefault [ext], as driven by /root/reference/src/main_ksp.cpp:92-103
// (KSPCG, KSPSetReusePreconditioner) and the options of
// /root/reference/configs/PETSc_SolverOptions_GAMG.info. Per iteration:
//
//   K1  P = Z            (i = 0)      | P = Z + b P        (VecCopy / VecAYPX)
//   K2  W = A P, partials of P.W      (KSP_MatMult + VecXDot, fused into the
//                                      STREAM SpMV epilogue when possible)
//   K3  scalar step: dpi, indefinite-matrix check, a = beta / dpi
//   K4  X += a P, R -= a W            (2 x VecAXPY), and for Jacobi / none
//       also Z = D^-1 R with the partials of Z.Z, Z.R, R.R fused in
//   [GAMG: Z = V-cycle(R), then the Z.Z, Z.R partials]
//   K5  scalar step: dp, KSPConvergedDefault, beta, indefinite-PC / beta = 0
//                    checks, b = beta / betaold
//
// W shares Z's storage as in PETSc (W = Z when not single-reduction). All
// scalars live on the device; kernels return at once once the device flag
// `done` is set, so the host launches iterations in batches and polls.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "aijhip_gamg.h"
#include "gamg_device.h"
#include "aijhip_internal.h"
#include "aijhip_ksp.h"
#include "cg_device.h"

namespace {

// K3 / K5 / init: this device's partials summed in a fixed order, then the
// scalar step (cg_device.h).
__global__ __launch_bounds__(kRedThreads) void k_reduce_init(const double *part, int nb, CGState *S,
                                                             double *hist, CGParams p) {
    __shared__ double scratch[kRedThreads / 64];
    const double zz = reduce_parts(part + 0 * nb, nb, scratch);
    const double zr = reduce_parts(part + 1 * nb, nb, scratch);
    const double rr = reduce_parts(part + 2 * nb, nb, scratch);
    const double ss = reduce_parts(part + 3 * nb, nb, scratch);
    if (threadIdx.x == 0) step_init(zz, zr, rr, ss, S, hist, p);
}

__global__ __launch_bounds__(kRedThreads) void k_reduce_dpi(const double *part, int nb, CGState *S) {
    __shared__ double scratch[kRedThreads / 64];
    if (S->done) return;
    const double dpi = reduce_parts(part, nb, scratch);
    if (threadIdx.x == 0) step_dpi(dpi, S);
}

// zz, zr come from pz[0, nbz) and pz[nbz, 2 nbz) (the vector kernels' slots 0
// and 1, or the fused V-cycle's finest post-smoothing); rr from pr[0, nbr).
__global__ __launch_bounds__(kRedThreads) void k_reduce_iter(const double *pz, int nbz, const double *pr, int nbr,
                                                             CGState *S, double *hist, CGParams p) {
    __shared__ double scratch[kRedThreads / 64];
    if (S->done) return;
    const double zz = reduce_parts(pz, nbz, scratch);
    const double zr = reduce_parts(pz + nbz, nbz, scratch);
    const double rr = reduce_parts(pr, nbr, scratch);
    if (threadIdx.x == 0) step_iter(zz, zr, rr, S, hist, p);
}

// ------------------------------------------------------------- V-cycle
// KSPSolve_Richardson with one iteration, scale 1, Jacobi PC [ext]:
//   zero guess:     x = 0 + 1.0 * (D^-1 b)           = D^-1 b
//   nonzero guess:  x = x + 1.0 * (D^-1 (b + (-1) A x))
// Every V-cycle kernel takes CG's stop flag (`done`, NULL outside a solve):
// once it is set they return at once, so the solver can launch iterations in
// batches between host polls as CG+Jacobi does.
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

int kfail(int code, const std::string &msg) {
    aijhip::set_error(msg);
    return code;
}

int khip(hipError_t e, const char *what) {
    aijhip::set_error(std::string(what) + ": " + hipGetErrorString(e));
    return AIJHIP_ERR_HIP;
}

struct MGLevel {
    aijhip_mat *A = nullptr;  // level 0: borrowed
    aijhip_mat *P = nullptr;  // interpolation from level l+1 (owned)
    bool own_A = false;
    bool fused = false;       // smoothing passes fused into STREAM launches
    int32_t m = 0;
    int64_t nnz = 0;
    double *dinv = nullptr, *b = nullptr, *x = nullptr, *r = nullptr;
    double *tdinv = nullptr;  // row templates (the finest level): D^-1 per template
};

}  // namespace

struct aijhip_ksp {
    aijhip_mat *A = nullptr;
    int pc = AIJHIP_PC_JACOBI;
    int normtype = AIJHIP_KSP_NORM_PRECONDITIONED;
    bool guess_nonzero = false;
    double rtol = 1e-5, abstol = 1e-50, dtol = 1e5;
    int32_t max_it = 10000;
    aijhip_gamg_params_t gamg;
    bool set_up = false;
    uint64_t a_gen = 0;  // the operator's plan generation at set-up: a re-planned
                         // operator (options, MatAssemblyEnd) is set up again
    uint64_t v_gen = 0;  // its values generation: new values (aijhip_mat_update_values)
                         // redo the PC set-up (D^-1, the GAMG hierarchy)
    bool fused = false;
    int vec_grid = 0;
    // CG vector kernels store with the non-temporal hint (tools: CG+Jacobi
    // 1053 -> 1093 it/s). V-cycle pre-smoothing on fused levels is x = D^-1 b
    // as a vector pass, then r = b - A x in the SpMV epilogue (OpMgResid):
    // one launch gathering dinv_j * b_j solved in 0.221 s against 0.205 s
    // (profiles/r01/mg_pre_split/). X += a P is deferred into the next
    // p = z + b p pass: in the r/z update (PETSc's place) CG+Jacobi took
    // 0.392 s against 0.376 s per 400 iterations (profiles/r01/x_in_update/).
    // (Those A/B forms were withdrawn in round 4.)
    double *d_dinv = nullptr, *d_r = nullptr, *d_z = nullptr, *d_p = nullptr, *d_part = nullptr;
    // CG + Jacobi on row templates: D^-1 per template (d_tdinv, indexed by
    // the operator's template ids) and Z not stored (k_aypx / k_update IZ)
    double *d_tdinv = nullptr;
    bool implicit_z = false;
    double *d_hist = nullptr;
    double *d_hb = nullptr, *d_hx = nullptr;  // aijhip_ksp_solve_host's device copies of b and x
    int32_t hist_cap = 0;
    CGState *d_state = nullptr;
    CGState *h_state = nullptr;  // pinned
    std::vector<MGLevel> mg;     // GAMG levels, finest first
    double *d_mgpart = nullptr;  // fused finest-level z.z / z.r partials
    double setup_seconds = 0.0;
    // how each level's coarsening was built (aijhip_ksp_get_gamg_setup_path)
    std::vector<int32_t> setup_path, setup_cols;
    bool setup_overflow = false;
    int32_t its = 0, host_syncs = 0;
    int reason = 0;
    double rnorm = 0.0;
    std::vector<double> hist;
};

namespace {

void mg_free(aijhip_ksp *K) {
    for (MGLevel &L : K->mg) {
        if (L.own_A) aijhip_mat_destroy(L.A);
        aijhip_mat_destroy(L.P);
        hipFree(L.dinv); hipFree(L.b); hipFree(L.x); hipFree(L.r); hipFree(L.tdinv);
    }
    K->mg.clear();
    hipFree(K->d_mgpart);
    K->d_mgpart = nullptr;
}

void ksp_free(aijhip_ksp *K) {
    mg_free(K);
    hipFree(K->d_dinv); hipFree(K->d_r); hipFree(K->d_z); hipFree(K->d_p); hipFree(K->d_part);
    hipFree(K->d_tdinv);
    K->d_tdinv = nullptr;
    K->implicit_z = false;
    hipFree(K->d_hist); hipFree(K->d_state);
    hipFree(K->d_hb); hipFree(K->d_hx);
    K->d_hb = K->d_hx = nullptr;
    if (K->h_state) hipHostFree(K->h_state);
    K->d_dinv = K->d_r = K->d_z = K->d_p = K->d_part = K->d_hist = nullptr;
    K->d_state = nullptr;
    K->h_state = nullptr;
    K->set_up = false;
}

struct KDeviceGuard {
    int prev = -1;
    explicit KDeviceGuard(int dev) {
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur != dev && hipSetDevice(dev) == hipSuccess) prev = cur;
    }
    ~KDeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

dim3 vgrid(const aijhip_ksp *K, int64_t n) {
    return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kVecThreads - 1) / kVecThreads,
                                                                 (int64_t)K->A->n_cu * 8)));
}

// PCSetUp_GAMG. The large levels are built on the device
// (aijhip_gamg::build_device: strength graph, emax, smoothing and Galerkin
// product on the GPU, greedy aggregation on the host); the hierarchy below
// device_min_rows rows (or past the device accumulators) continues on the
// host from that level's operator and near-null space. Either way the
// levels equal aijhip_gamg_build_host's bit for bit. AIJHIP_GAMG_LOG=1 prints
// the phases.
int gamg_setup(aijhip_ksp *K) {
    aijhip::Range range("PCSetUp_GAMG");
    aijhip_mat *A = K->A;
    const bool log = std::getenv("AIJHIP_GAMG_LOG") != nullptr;
    auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!log) return;
        (void)hipDeviceSynchronize();
        const auto t = std::chrono::steady_clock::now();
        std::fprintf(stderr, "gamg set-up %-22s %8.3f s\n", what, std::chrono::duration<double>(t - t0).count());
        t0 = t;
    };
    std::vector<aijhip_gamg::DeviceLevel> dl;
    std::vector<double> B;
    bool more = false, overflow = false;
    int rc = aijhip_gamg::build_device(A, K->gamg, dl, B, &more, &overflow);
    if (rc) return rc;
    K->setup_path.clear();
    K->setup_cols.clear();
    for (size_t l = 0; l + 1 < dl.size(); ++l) {
        K->setup_path.push_back(1);
        K->setup_cols.push_back(dl[l].product_cols);
    }
    K->setup_overflow = overflow;
    lap("device levels");
    hipError_t e = hipSuccess;
    aijhip_gamg_host_t H = nullptr;
    int32_t nh = 0;
    if (more) {  // host continuation from the last device level
        const aijhip_mat &L = *dl.back().A;
        std::vector<int32_t> ai((size_t)L.m + 1), aj((size_t)L.nz);
        std::vector<double> aa((size_t)L.nz);
        if ((e = hipMemcpy(ai.data(), L.d_ai, sizeof(int32_t) * ai.size(), hipMemcpyDeviceToHost)) != hipSuccess ||
            (L.nz > 0 &&
             ((e = hipMemcpy(aj.data(), L.d_aj, sizeof(int32_t) * (size_t)L.nz, hipMemcpyDeviceToHost)) != hipSuccess ||
              (e = hipMemcpy(aa.data(), L.d_aa, sizeof(double) * (size_t)L.nz, hipMemcpyDeviceToHost)) != hipSuccess))) {
            aijhip_gamg::free_device_levels(dl);
            return khip(e, "GAMG: read level operator");
        }
        aijhip_gamg_params_t hp = K->gamg;
        hp.max_levels = K->gamg.max_levels - ((int32_t)dl.size() - 1);
        const int32_t nd_levels = (int32_t)dl.size();  // the host continues at level nd_levels - 1
        rc = aijhip_gamg::build_host_nns(L.m, ai.data(), aj.data(), aa.data(), B.data(), hp, &H, nd_levels - 1);
        if (rc) {
            aijhip_gamg::free_device_levels(dl);
            return kfail(rc, "GAMG: host hierarchy set-up failed");
        }
        aijhip_gamg_host_num_levels(H, &nh);
        lap("host levels");
    }
    const int32_t nd = (int32_t)dl.size();
    const int32_t nl = nd + (nh > 0 ? nh - 1 : 0);
    for (int32_t hl = 1; hl < nh; ++hl) {
        K->setup_path.push_back(0);
        K->setup_cols.push_back(-1);
    }
    K->mg.assign((size_t)nl, MGLevel());
    for (int32_t l = 0; l < nd; ++l) {  // the device levels move into the KSP
        K->mg[l].A = dl[l].A;
        K->mg[l].own_A = l > 0;
        K->mg[l].P = dl[l].P;
    }
    dl.clear();
    for (int32_t hl = 1; hl < nh && !rc; ++hl) {  // host level hl = level nd - 1 + hl
        MGLevel &L = K->mg[nd - 1 + hl];
        MGLevel &U = K->mg[nd - 2 + hl];
        int32_t mu = 0, mc = 0;
        int64_t nnz_a = 0, nnz_p = 0;
        aijhip_gamg_host_level_info(H, hl - 1, &mu, nullptr, &nnz_p, nullptr);
        aijhip_gamg_host_level_info(H, hl, &mc, &nnz_a, nullptr, nullptr);
        const int32_t *xi, *xj;
        const double *xa;
        aijhip_gamg_host_view(H, hl - 1, 'P', &xi, &xj, &xa);
        rc = aijhip_mat_create(A->device, mu, mc, nnz_p, xi, xj, xa, &U.P);
        if (rc) break;
        aijhip_gamg_host_view(H, hl, 'A', &xi, &xj, &xa);
        rc = aijhip_mat_create(A->device, mc, mc, nnz_a, xi, xj, xa, &L.A);
        L.own_A = rc == AIJHIP_OK;
    }
    if (H) aijhip_gamg_host_destroy(H);
    if (rc) return rc;
    for (int32_t l = 0; l < nl; ++l) {
        MGLevel &L = K->mg[l];
        L.m = L.A->m;
        L.nnz = L.A->nz;
        const size_t vb = sizeof(double) * (size_t)std::max<int32_t>(L.m, 1);
        if ((e = hipMalloc(&L.dinv, vb)) != hipSuccess || (e = hipMalloc(&L.r, vb)) != hipSuccess ||
            (l > 0 && ((e = hipMalloc(&L.b, vb)) != hipSuccess || (e = hipMalloc(&L.x, vb)) != hipSuccess)))
            return khip(e, "GAMG: level vectors");
        if (L.m > 0)
            hipLaunchKernelGGL(k_diag_inv, dim3((unsigned)((L.m + 255) / 256)), dim3(256), 0, nullptr, L.m,
                               L.A->d_ai, L.A->d_aj, L.A->d_aa, L.dinv);
        // the finest level on row templates: D^-1 per template for its fused
        // smoothing (pre-smoothing pass and post-smoothing epilogue read a
        // template id instead of D^-1; AIJHIP_KSP_EXPLICIT_Z=1 keeps dinv)
        if (l == 0 && L.m > 0 && L.A->plan.d_pid && L.A->plan.d_pval && !std::getenv("AIJHIP_KSP_EXPLICIT_Z")) {
            const int np = L.A->plan.n_pat;
            if ((e = hipMalloc(&L.tdinv, sizeof(double) * (size_t)np)) != hipSuccess)
                return khip(e, "GAMG: template D^-1");
            hipLaunchKernelGGL(k_tmpl_dinv, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, nullptr, np,
                               L.A->plan.d_ptab, L.A->plan.d_pval, L.tdinv);
        }
    }
    // every restriction (P^T) exists before the first solve (the device
    // levels attached theirs during the set-up)
    for (int32_t l = 0; l + 1 < nl; ++l) {
        MGLevel &L = K->mg[l];
        if (!L.P->transpose && (rc = aijhip_mat_mult_transpose(L.P, L.r, K->mg[l + 1].b, nullptr))) return rc;
    }
    for (MGLevel &L : K->mg) L.fused = !std::getenv("AIJHIP_MG_UNFUSED") && aijhip::stream_mg_fusable(*L.A);
    if (K->mg[0].fused &&
        (e = hipMalloc(&K->d_mgpart, sizeof(double) * 2 * (size_t)std::max(1, K->mg[0].A->plan.n_blocks))) !=
            hipSuccess)
        return khip(e, "GAMG partials");
    if ((e = hipDeviceSynchronize()) != hipSuccess) return khip(e, "GAMG set-up");
    lap("level vectors, P^T");
    return AIJHIP_OK;
}

// PCApply_MG (multiplicative, one V-cycle) on the finest-level input b,
// output x. On STREAM-planned levels the smoothing passes ride in the SpMV
// (aijhip::launch_mg_resid / _post): the residual rides in the SpMV after
// the x = D^-1 b vector pass,
// and interpolation writes t = x + P x_c to the level's scratch so the
// post-smoothing launch reads t and writes x. With dots != NULL the finest
// post-smoothing also leaves z.z / z.b partials there (*dots_done = true).
hipError_t vcycle(aijhip_ksp *K, const double *b0, double *x0, hipStream_t s, double *dots = nullptr,
                  bool *dots_done = nullptr, const int *stop = nullptr) {
    const int nl = (int)K->mg.size();
    hipError_t e = hipSuccess;
    if (dots_done) *dots_done = false;
    auto B = [&](int l) { return l == 0 ? b0 : (const double *)K->mg[l].b; };
    auto X = [&](int l) { return l == 0 ? x0 : K->mg[l].x; };
    for (int l = 0; l < nl; ++l) {
        MGLevel &L = K->mg[l];
        const dim3 g = vgrid(K, L.m), t(kVecThreads);
        if (l == nl - 1) {  // coarse: preonly + Jacobi
            hipLaunchKernelGGL(k_jacobi, g, t, 0, s, (int64_t)L.m, L.dinv, B(l), X(l), stop);
            break;
        }
        if (L.fused) {
            // smoothd as a vector pass, then r = b - A x in the SpMV epilogue
            if (L.tdinv)
                hipLaunchKernelGGL(k_jacobi_t, g, t, 0, s, (int64_t)L.m, L.A->plan.d_pid, L.tdinv, B(l), X(l), stop);
            else
                hipLaunchKernelGGL(k_jacobi, g, t, 0, s, (int64_t)L.m, L.dinv, B(l), X(l), stop);
            if ((e = aijhip::launch_mg_resid(*L.A, X(l), B(l), L.r, s, stop)) != hipSuccess) return e;
        } else {
            hipLaunchKernelGGL(k_jacobi, g, t, 0, s, (int64_t)L.m, L.dinv, B(l), X(l), stop);  // smoothd
            if ((e = aijhip::launch_mult(*L.A, X(l), nullptr, L.r, false, s, stop)) != hipSuccess) return e;
            hipLaunchKernelGGL(k_resid, g, t, 0, s, (int64_t)L.m, B(l), L.r, stop);
        }
        if ((e = aijhip::launch_mult(*L.P->transpose, L.r, nullptr, K->mg[l + 1].b, false, s, stop)) != hipSuccess)
            return e;  // MatRestrict = P^T r
    }
    for (int l = nl - 2; l >= 0; --l) {
        MGLevel &L = K->mg[l];
        const dim3 g = vgrid(K, L.m), t(kVecThreads);
        if (L.fused) {
            // MatInterpolateAdd into the scratch: t = x + P x_c, then smoothu
            if ((e = aijhip::launch_mult(*L.P, X(l + 1), X(l), L.r, true, s, stop)) != hipSuccess) return e;
            double *dp = (l == 0 && dots) ? dots : nullptr;
            if ((e = aijhip::launch_mg_post(*L.A, L.r, B(l), L.dinv, X(l), dp, s, stop, L.tdinv)) != hipSuccess)
                return e;
            if (dp && dots_done) *dots_done = true;
        } else {
            // MatInterpolateAdd: x = x + P x_c
            if ((e = aijhip::launch_mult(*L.P, X(l + 1), X(l), X(l), true, s, stop)) != hipSuccess) return e;
            if ((e = aijhip::launch_mult(*L.A, X(l), nullptr, L.r, false, s, stop)) != hipSuccess) return e;
            hipLaunchKernelGGL(k_richardson, g, t, 0, s, (int64_t)L.m, L.dinv, B(l), L.r, X(l), stop);  // smoothu
        }
    }
    return hipGetLastError();
}

}  // namespace

namespace aijhip {

hipError_t ksp_pc_vcycle(aijhip_ksp *K, const double *b, double *x, hipStream_t s, const double **dots,
                         int *nbz, const int *stop) {
    bool done = false;
    const hipError_t e = vcycle(K, b, x, s, K->d_mgpart, &done, stop);
    *dots = done ? K->d_mgpart : nullptr;
    *nbz = done ? K->mg[0].A->plan.n_blocks : 0;
    return e;
}

}  // namespace aijhip

extern "C" {

int aijhip_ksp_create(aijhip_mat_t A, aijhip_ksp_t *out) {
    if (!out) return kfail(AIJHIP_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!A) return kfail(AIJHIP_ERR_ARG, "NULL matrix");
    if (A->m != A->n) return kfail(AIJHIP_ERR_ARG, "CG needs a square operator");
    aijhip_ksp *K = new (std::nothrow) aijhip_ksp();
    if (!K) return kfail(AIJHIP_ERR_ALLOC, "host allocation");
    K->A = A;
    aijhip_gamg_params_default(&K->gamg);
    *out = K;
    return AIJHIP_OK;
}

int aijhip_ksp_set_tolerances(aijhip_ksp_t K, double rtol, double abstol, double dtol, int32_t max_it) {
    if (!K) return kfail(AIJHIP_ERR_ARG, "NULL ksp");
    if (rtol < 0 || abstol < 0 || dtol <= 0 || max_it < 0) return kfail(AIJHIP_ERR_ARG, "bad tolerance");
    K->rtol = rtol; K->abstol = abstol; K->dtol = dtol;
    if (max_it != K->max_it) {
        K->max_it = max_it;
        if (K->set_up && K->hist_cap < max_it + 2) {  // regrow the history only
            hipFree(K->d_hist);
            K->d_hist = nullptr;
            K->hist_cap = max_it + 2;
            if (hipMalloc(&K->d_hist, sizeof(double) * (size_t)K->hist_cap) != hipSuccess) {
                K->set_up = false;
                return kfail(AIJHIP_ERR_ALLOC, "residual history");
            }
        }
    }
    return AIJHIP_OK;
}

int aijhip_ksp_set_pc_type(aijhip_ksp_t K, int pc) {
    if (!K) return kfail(AIJHIP_ERR_ARG, "NULL ksp");
    if (pc != AIJHIP_PC_NONE && pc != AIJHIP_PC_JACOBI && pc != AIJHIP_PC_GAMG)
        return kfail(AIJHIP_ERR_ARG, "unknown PC type");
    if (pc != K->pc) K->set_up = false;
    K->pc = pc;
    if (pc == AIJHIP_PC_GAMG)  // the set-up's streams, made once per process
        for (int slot = 0; slot < 2; ++slot) (void)aijhip_gamg::setup_stream(K->A->device, slot);
    return AIJHIP_OK;
}

int aijhip_ksp_set_gamg_params(aijhip_ksp_t K, const aijhip_gamg_params_t *p) {
    if (!K) return kfail(AIJHIP_ERR_ARG, "NULL ksp");
    if (p) K->gamg = *p;
    else aijhip_gamg_params_default(&K->gamg);
    if (K->pc == AIJHIP_PC_GAMG) K->set_up = false;
    return AIJHIP_OK;
}

int aijhip_ksp_set_norm_type(aijhip_ksp_t K, int nt) {
    if (!K) return kfail(AIJHIP_ERR_ARG, "NULL ksp");
    if (nt < AIJHIP_KSP_NORM_NONE || nt > AIJHIP_KSP_NORM_NATURAL) return kfail(AIJHIP_ERR_ARG, "bad norm type");
    K->normtype = nt;
    return AIJHIP_OK;
}

int aijhip_ksp_set_initial_guess_nonzero(aijhip_ksp_t K, int flg) {
    if (!K) return kfail(AIJHIP_ERR_ARG, "NULL ksp");
    K->guess_nonzero = flg != 0;
    return AIJHIP_OK;
}

int aijhip_ksp_set_up(aijhip_ksp_t K) {
    aijhip::Range range("KSPSetUp");
    if (!K) return kfail(AIJHIP_ERR_ARG, "NULL ksp");
    if (K->set_up && K->a_gen == K->A->plan_gen && K->v_gen == K->A->values_gen) return AIJHIP_OK;
    const auto t0 = std::chrono::steady_clock::now();
    aijhip_mat *A = K->A;
    KDeviceGuard g(A->device);
    ksp_free(K);
    const int64_t m = A->m;
    const size_t vb = sizeof(double) * (size_t)std::max<int64_t>(m, 1);
    K->fused = aijhip::stream_dot_fusable(*A);
    K->vec_grid = (int)vgrid(K, m).x;
    const int64_t nparts = std::max<int64_t>((int64_t)kNQ * K->vec_grid, K->fused ? A->plan.n_blocks : K->vec_grid);
    K->hist_cap = K->max_it + 2;
    hipError_t e;
    if ((e = hipMalloc(&K->d_dinv, vb)) != hipSuccess || (e = hipMalloc(&K->d_r, vb)) != hipSuccess ||
        (e = hipMalloc(&K->d_z, vb)) != hipSuccess || (e = hipMalloc(&K->d_p, vb)) != hipSuccess ||
        (e = hipMalloc(&K->d_part, sizeof(double) * (size_t)nparts)) != hipSuccess ||
        (e = hipMalloc(&K->d_hist, sizeof(double) * (size_t)K->hist_cap)) != hipSuccess ||
        (e = hipMalloc(&K->d_state, sizeof(CGState))) != hipSuccess ||
        (e = hipHostMalloc(&K->h_state, sizeof(CGState), hipHostMallocDefault)) != hipSuccess) {
        ksp_free(K);
        return khip(e, "ksp set-up allocation");
    }
    if (m > 0) {
        hipLaunchKernelGGL(k_diag_inv, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, nullptr, A->m, A->d_ai,
                           A->d_aj, A->d_aa, K->d_dinv);
        if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) {
            ksp_free(K);
            return khip(e, "PCSetUp_Jacobi");
        }
    }
    // Jacobi on row templates: D^-1 per template, Z formed where it is read
    // (AIJHIP_KSP_EXPLICIT_Z=1 keeps the stored Z, for A/B)
    if (K->pc == AIJHIP_PC_JACOBI && m > 0 && A->plan.d_pid && A->plan.d_pval && !std::getenv("AIJHIP_KSP_EXPLICIT_Z")) {
        const int np = A->plan.n_pat;
        if ((e = hipMalloc(&K->d_tdinv, sizeof(double) * (size_t)np)) != hipSuccess) {
            ksp_free(K);
            return khip(e, "PCSetUp_Jacobi (templates)");
        }
        hipLaunchKernelGGL(k_tmpl_dinv, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, nullptr, np,
                           A->plan.d_ptab, A->plan.d_pval, K->d_tdinv);
        if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess) {
            ksp_free(K);
            return khip(e, "PCSetUp_Jacobi (templates)");
        }
        K->implicit_z = true;
    }
    if (K->pc == AIJHIP_PC_GAMG) {
        const int rc = gamg_setup(K);
        if (rc) {
            ksp_free(K);
            return rc;
        }
    }
    K->setup_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    K->set_up = true;
    K->a_gen = A->plan_gen;
    K->v_gen = A->values_gen;
    return AIJHIP_OK;
}

int aijhip_ksp_solve(aijhip_ksp_t K, const double *b, double *x, void *stream) {
    aijhip::Range range("KSPSolve");
    if (!K) return kfail(AIJHIP_ERR_ARG, "NULL ksp");
    int rc = aijhip_ksp_set_up(K);
    if (rc) return rc;
    aijhip_mat *A = K->A;
    const int64_t m = A->m;
    if (m > 0 && (!b || !x)) return kfail(AIJHIP_ERR_ARG, "NULL vector");
    if (b == x) return kfail(AIJHIP_ERR_ARG, "b and x alias");
    KDeviceGuard g(A->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipError_t e = hipSuccess;
    const bool gamg = K->pc == AIJHIP_PC_GAMG;
    CGParams p{K->rtol, K->abstol, K->dtol, K->max_it, K->normtype, K->guess_nonzero ? 0 : 1, K->pc};
    const dim3 vg(K->vec_grid), vt(kVecThreads), rt(kRedThreads);
    const int nb = K->vec_grid;
    // KSPSolve [ext]: zero initial guess -> x = 0; else r = A x first.
    if (!K->guess_nonzero) {
        if (m > 0) e = hipMemsetAsync(x, 0, sizeof(double) * (size_t)m, s);
    } else {
        e = aijhip::launch_mult(*A, x, nullptr, K->d_r, false, s);
    }
    if (e != hipSuccess) return khip(e, "KSPSolve init");
    hipLaunchKernelGGL(k_init, vg, vt, 0, s, m, b, K->d_r, K->d_z, K->d_dinv, K->d_part, p);
    if (gamg) {
        if (K->guess_nonzero && K->normtype != AIJHIP_KSP_NORM_UNPRECONDITIONED) {
            // snorm = |B b| for the preconditioned-norm convergence test
            if ((e = vcycle(K, b, K->d_z, s)) != hipSuccess) return khip(e, "GAMG V-cycle");
            hipLaunchKernelGGL(k_dots, vg, vt, 0, s, m, K->d_z, nullptr, K->d_part, 3, -1, nullptr);
        }
        if ((e = vcycle(K, K->d_r, K->d_z, s)) != hipSuccess) return khip(e, "GAMG V-cycle");
        hipLaunchKernelGGL(k_dots, vg, vt, 0, s, m, K->d_z, K->d_r, K->d_part, 0, 1, nullptr);
    }
    hipLaunchKernelGGL(k_reduce_init, dim3(1), rt, 0, s, K->d_part, nb, K->d_state, K->d_hist, p);
    if ((e = hipGetLastError()) != hipSuccess) return khip(e, "KSPSolve init");
    // One CG iteration (+ the V-cycle) on stream st; every kernel is a
    // no-op once `done` is set.
    auto iterate = [&](hipStream_t st) -> hipError_t {
        hipError_t ie = hipSuccess;
        if (K->implicit_z)
            hipLaunchKernelGGL((k_aypx<true, true>), vg, vt, 0, st, m, K->d_z, K->d_p, x, K->d_state, K->d_r,
                               A->plan.d_pid, K->d_tdinv);
        else
            hipLaunchKernelGGL(k_aypx<true>, vg, vt, 0, st, m, K->d_z, K->d_p, x, K->d_state);
        if (K->fused) {
            ie = aijhip::launch_stream_dot(*A, K->d_p, K->d_z, K->d_part, &K->d_state->done, st);
            if (ie == hipSuccess)
                hipLaunchKernelGGL(k_reduce_dpi, dim3(1), rt, 0, st, K->d_part, A->plan.n_blocks, K->d_state);
        } else {
            ie = aijhip::launch_mult(*A, K->d_p, nullptr, K->d_z, false, st, &K->d_state->done);
            hipLaunchKernelGGL(k_dot, vg, vt, 0, st, m, K->d_p, K->d_z, K->d_part, K->d_state);
            hipLaunchKernelGGL(k_reduce_dpi, dim3(1), rt, 0, st, K->d_part, nb, K->d_state);
        }
        if (K->implicit_z)
            hipLaunchKernelGGL((k_update<true, true>), vg, vt, 0, st, m, K->d_r, K->d_z, K->d_dinv, K->d_part,
                               K->d_state, K->pc, K->d_p, nullptr, A->plan.d_pid, K->d_tdinv);
        else
            hipLaunchKernelGGL(k_update<true>, vg, vt, 0, st, m, K->d_r, K->d_z, K->d_dinv, K->d_part, K->d_state,
                               K->pc, K->d_p, nullptr);
        const double *pz = K->d_part;
        int nbz = nb;
        if (gamg && ie == hipSuccess) {
            // z = B r; z.z and z.r come from the finest post-smoothing
            // when it is fused, else from k_dots
            bool dots = false;
            ie = vcycle(K, K->d_r, K->d_z, st, K->d_mgpart, &dots, &K->d_state->done);
            if (dots) {
                pz = K->d_mgpart;
                nbz = K->mg[0].A->plan.n_blocks;
            } else {
                hipLaunchKernelGGL(k_dots, vg, vt, 0, st, m, K->d_z, K->d_r, K->d_part, 0, 1, K->d_state);
            }
        }
        hipLaunchKernelGGL(k_reduce_iter, dim3(1), rt, 0, st, pz, nbz, K->d_part + 2 * nb, nb, K->d_state,
                           K->d_hist, p);
        return ie != hipSuccess ? ie : hipGetLastError();
    };
    // iterations in batches between polls (AIJHIP_KSP_POLL overrides the
    // batch, for A/B). The kernels run back to back (a kernel trace of the
    // 300^3 CG + GAMG solve: busy 0.996 of its span), and a batch replayed as
    // one captured HIP graph measured slower (solve 0.194 vs 0.188 s, CG +
    // Jacobi 0.331 vs 0.325 s per 400 iterations: profiles/r04/s1/graph_ab.txt)
    int batch = 8;
    if (const char *v = std::getenv("AIJHIP_KSP_POLL")) batch = std::max(1, std::atoi(v));
    int32_t launched = 0;
    K->host_syncs = 0;
    for (;;) {
        ++K->host_syncs;
        if ((e = hipMemcpyAsync(K->h_state, K->d_state, sizeof(CGState), hipMemcpyDeviceToHost, s)) != hipSuccess ||
            (e = hipStreamSynchronize(s)) != hipSuccess)
            return khip(e, "KSPSolve poll");
        if (K->h_state->done || launched >= K->max_it) break;
        for (int j = 0; j < batch && launched < K->max_it; ++j, ++launched)
            if ((e = iterate(s)) != hipSuccess) return khip(e, "KSPSolve iteration");
    }
    hipLaunchKernelGGL(k_final_x, vg, vt, 0, s, m, K->d_p, x, K->d_state);
    if ((e = hipGetLastError()) != hipSuccess ||
        (e = hipMemcpyAsync(K->h_state, K->d_state, sizeof(CGState), hipMemcpyDeviceToHost, s)) != hipSuccess ||
        (e = hipStreamSynchronize(s)) != hipSuccess)
        return khip(e, "KSPSolve final update");
    ++K->host_syncs;
    const CGState &st = *K->h_state;
    K->its = st.its;
    K->reason = st.reason ? st.reason : AIJHIP_KSP_DIVERGED_ITS;
    K->rnorm = st.dp;
    const int32_t nh = std::min<int32_t>(K->hist_cap, st.its + 1);
    K->hist.resize((size_t)std::max(nh, 0));
    if (nh > 0 &&
        (e = hipMemcpy(K->hist.data(), K->d_hist, sizeof(double) * (size_t)nh, hipMemcpyDeviceToHost)) != hipSuccess)
        return khip(e, "residual history");
    return AIJHIP_OK;
}

int aijhip_ksp_get_iteration_number(aijhip_ksp_t K, int32_t *its) {
    if (!K || !its) return kfail(AIJHIP_ERR_ARG, "NULL argument");
    *its = K->its;
    return AIJHIP_OK;
}

int aijhip_ksp_get_residual_norm(aijhip_ksp_t K, double *rnorm) {
    if (!K || !rnorm) return kfail(AIJHIP_ERR_ARG, "NULL argument");
    *rnorm = K->rnorm;
    return AIJHIP_OK;
}

int aijhip_ksp_get_converged_reason(aijhip_ksp_t K, int *reason) {
    if (!K || !reason) return kfail(AIJHIP_ERR_ARG, "NULL argument");
    *reason = K->reason;
    return AIJHIP_OK;
}

int aijhip_ksp_get_residual_history(aijhip_ksp_t K, double *hist, int32_t na, int32_t *n) {
    if (!K || !n || (na > 0 && !hist)) return kfail(AIJHIP_ERR_ARG, "NULL argument");
    const int32_t c = std::min<int32_t>(na, (int32_t)K->hist.size());
    std::copy(K->hist.begin(), K->hist.begin() + c, hist);
    *n = c;
    return AIJHIP_OK;
}

int aijhip_ksp_get_host_syncs(aijhip_ksp_t K, int32_t *n) {
    if (!K || !n) return kfail(AIJHIP_ERR_ARG, "NULL argument");
    *n = K->host_syncs;
    return AIJHIP_OK;
}

int aijhip_ksp_get_iteration_bytes(aijhip_ksp_t K, int64_t *bytes, int64_t *spmv_bytes, int64_t *level0) {
    if (!K || !bytes) return kfail(AIJHIP_ERR_ARG, "NULL argument");
    if (!K->set_up) return kfail(AIJHIP_ERR_STATE, "KSP is not set up");
    const int64_t m = K->A->m;
    const int64_t a0 = aijhip::mult_layout_bytes(*K->A);
    // CG: p = z + b p with x += a p (reads z, p, x; writes p, x), the SpMV
    // (p . w in its epilogue), the r update (Jacobi: reads r, w, D^-1,
    // writes r, z; GAMG: reads r, w, writes r; z from the V-cycle)
    // (Jacobi on row templates, Z not stored: p = z + b p reads r and a
    // template id instead of z; the update reads r, w and an id, writes r)
    int64_t spmv = a0, vec = K->implicit_z ? 41 * m + 25 * m : 40 * m + (K->pc == AIJHIP_PC_GAMG ? 24 * m : 40 * m);
    if (!K->fused) vec += 16 * m;  // p . w in its own pass
    int64_t lev0 = a0 + vec;
    if (K->pc == AIJHIP_PC_GAMG) {
        const int nl = (int)K->mg.size();
        for (int l = 0; l < nl; ++l) {
            const MGLevel &L = K->mg[l];
            const int64_t ml = L.m;
            int64_t sp = 0, v = 0;
            if (l == nl - 1) {
                v = 24 * ml;  // coarse: x = D^-1 b
            } else {
                const int64_t la = aijhip::mult_layout_bytes(*L.A);
                const int64_t lp = aijhip::mult_layout_bytes(*L.P);
                const int64_t lt = L.P->transpose ? aijhip::mult_layout_bytes(*L.P->transpose) : lp;
                if (L.fused && L.tdinv)  // the same with a template id for D^-1 (two passes)
                    sp = la + lt + lp + la, v = 17 * ml + 8 * ml + 8 * ml + 9 * ml;
                else if (L.fused)  // D^-1 b pass; r = b - A x (+ b); P^T r; t = x + P x_c (+ x); x = t + D^-1 (b - A t) (+ b, D^-1)
                    sp = la + lt + lp + la, v = 24 * ml + 8 * ml + 8 * ml + 16 * ml;
                else  // the same with the residual and Richardson passes separate
                    sp = la + lt + lp + la, v = 24 * ml + 24 * ml + 8 * ml + 40 * ml;
            }
            spmv += sp;
            vec += v;
            if (l == 0) lev0 += sp + v;
        }
    }
    *bytes = spmv + vec;
    if (spmv_bytes) *spmv_bytes = spmv;
    if (level0) *level0 = lev0;
    return AIJHIP_OK;
}

int aijhip_ksp_get_fused(aijhip_ksp_t K, int *fused) {
    if (!K || !fused) return kfail(AIJHIP_ERR_ARG, "NULL argument");
    *fused = K->fused ? 1 : 0;
    return AIJHIP_OK;
}

int aijhip_ksp_get_pc_levels(aijhip_ksp_t K, int32_t *nlevels, int32_t *rows, int64_t *nnz, int32_t cap,
                             double *setup_seconds) {
    if (!K || !nlevels) return kfail(AIJHIP_ERR_ARG, "NULL argument");
    if (K->mg.empty()) {
        *nlevels = 1;
        if (cap > 0 && rows) rows[0] = K->A->m;
        if (cap > 0 && nnz) nnz[0] = K->A->nz;
    } else {
        *nlevels = (int32_t)K->mg.size();
        for (int32_t l = 0; l < std::min<int32_t>(cap, *nlevels); ++l) {
            if (rows) rows[l] = K->mg[l].m;
            if (nnz) nnz[l] = K->mg[l].nnz;
        }
    }
    if (setup_seconds) *setup_seconds = K->setup_seconds;
    return AIJHIP_OK;
}

int aijhip_ksp_get_pc_level(aijhip_ksp_t K, int32_t l, char which, int32_t *m, int32_t *n, int64_t *nnz,
                            int32_t *ai, int32_t *aj, double *aa) {
    if (!K || l < 0 || l >= (int32_t)K->mg.size() || (which != 'A' && which != 'P'))
        return kfail(AIJHIP_ERR_ARG, "no such PC level (set up a GAMG KSP first)");
    const aijhip_mat *M = which == 'A' ? K->mg[l].A : K->mg[l].P;
    if (!M) return kfail(AIJHIP_ERR_ARG, "the coarsest level has no interpolation");
    if (m) *m = M->m;
    if (n) *n = M->n;
    if (nnz) *nnz = M->nz;
    if (!ai) return AIJHIP_OK;
    KDeviceGuard g(M->device);
    hipError_t e = hipMemcpy(ai, M->d_ai, sizeof(int32_t) * ((size_t)M->m + 1), hipMemcpyDeviceToHost);
    if (e == hipSuccess && aj && M->nz > 0) e = hipMemcpy(aj, M->d_aj, sizeof(int32_t) * (size_t)M->nz, hipMemcpyDeviceToHost);
    if (e == hipSuccess && aa && M->nz > 0) e = hipMemcpy(aa, M->d_aa, sizeof(double) * (size_t)M->nz, hipMemcpyDeviceToHost);
    return e == hipSuccess ? AIJHIP_OK : khip(e, "read PC level");
}

int aijhip_ksp_get_gamg_setup_path(aijhip_ksp_t K, int32_t cap, int32_t *path, int32_t *product_cols,
                                   int32_t *host_fallback) {
    if (!K) return kfail(AIJHIP_ERR_ARG, "null ksp");
    if (!K->set_up || K->pc != AIJHIP_PC_GAMG) return kfail(AIJHIP_ERR_STATE, "GAMG not set up");
    const size_t n = std::min<size_t>(K->setup_path.size(), (size_t)std::max(cap, 0));
    for (size_t l = 0; l < n; ++l) {
        if (path) path[l] = K->setup_path[l];
        if (product_cols) product_cols[l] = K->setup_cols[l];
    }
    if (host_fallback) *host_fallback = K->setup_overflow ? 1 : 0;
    return AIJHIP_OK;
}

int aijhip_ksp_solve_host(aijhip_ksp_t K, const double *b, double *x) {
    if (!K) return kfail(AIJHIP_ERR_ARG, "NULL ksp");
    const int64_t m = K->A->m;
    if (m > 0 && (!b || !x)) return kfail(AIJHIP_ERR_ARG, "NULL vector");
    if (b == x) return kfail(AIJHIP_ERR_ARG, "b and x alias");
    int rc = aijhip_ksp_set_up(K);
    if (rc) return rc;
    KDeviceGuard g(K->A->device);
    hipError_t e = hipSuccess;
    if (!K->d_hb && (e = hipMalloc(&K->d_hb, sizeof(double) * (size_t)std::max<int64_t>(m, 1))) != hipSuccess)
        return khip(e, "KSPSolve host vectors");
    if (!K->d_hx && (e = hipMalloc(&K->d_hx, sizeof(double) * (size_t)std::max<int64_t>(m, 1))) != hipSuccess)
        return khip(e, "KSPSolve host vectors");
    // b (and a nonzero initial guess) up once, x down once: 2 x 8m bytes over
    // PCIe per solve instead of per MatMult (the reference's step-2 copies)
    if (m > 0 && ((e = hipMemcpy(K->d_hb, b, sizeof(double) * (size_t)m, hipMemcpyHostToDevice)) != hipSuccess ||
                  (K->guess_nonzero &&
                   (e = hipMemcpy(K->d_hx, x, sizeof(double) * (size_t)m, hipMemcpyHostToDevice)) != hipSuccess)))
        return khip(e, "KSPSolve b / x in");
    if ((rc = aijhip_ksp_solve(K, K->d_hb, K->d_hx, nullptr))) return rc;
    if (m > 0 && (e = hipMemcpy(x, K->d_hx, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost)) != hipSuccess)
        return khip(e, "KSPSolve x out");
    return AIJHIP_OK;
}

int aijhip_ksp_destroy(aijhip_ksp_t K) {
    if (!K) return AIJHIP_OK;
    {
        KDeviceGuard g(K->A->device);
        (void)hipDeviceSynchronize();
        ksp_free(K);
    }
    delete K;
    return AIJHIP_OK;
}

}  // extern "C"
