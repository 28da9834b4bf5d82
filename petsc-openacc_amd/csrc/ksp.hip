// ksp.hip — the single-GPU KSP handle (include/aijhip_ksp.h): KSPCG with PC
// none / Jacobi / GAMG on one aijhip_mat, as the reference's main_ksp drives
// it (KSPCG, KSPSetReusePreconditioner, PETSc_SolverOptions_GAMG.info).
//
// The CG itself is cg_solve.hip's driver and the V-cycle mg_cycle.hip's
// walker; this file is the handle, PCSetUp_GAMG, and what the handle plugs
// into the driver: the plain products (launch_stream_dot / launch_mult), no
// all-reduce, hipStreamSynchronize as the wait, and its hierarchy's V-cycle
// with the fused finest-level z.z / z.r partials.
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
#include "bcgs_solve.h"
#include "cg_multi.h"
#include "cg_solve.h"
#include "mg_cycle.h"

namespace {

// A level owns its operator, interpolation and vectors; what the V-cycle
// reads of it is the view it extends (m, D^-1, b / x / r, tdinv, fused).
struct MGLevel : aijhip::MGLevelView {
    aijhip_mat *A = nullptr;  // level 0: borrowed
    aijhip_mat *P = nullptr;  // interpolation from level l+1 (owned)
    bool own_A = false;
    int64_t nnz = 0;
};

}  // namespace

struct aijhip_ksp {
    aijhip_mat *A = nullptr;
    // The tolerances, CG's vectors and the last solve's results. The CG
    // vector kernels store with the non-temporal hint (tools: CG+Jacobi
    // 1053 -> 1093 it/s). V-cycle pre-smoothing on fused levels is x = D^-1 b
    // as a vector pass, then r = b - A x in the SpMV epilogue (OpMgResid):
    // one launch gathering dinv_j * b_j solved in 0.221 s against 0.205 s
    // (profiles/r01/mg_pre_split/). X += a P is deferred into the next
    // p = z + b p pass: in the r/z update (PETSc's place) CG+Jacobi took
    // 0.392 s against 0.376 s per 400 iterations (profiles/r01/x_in_update/).
    // (Those A/B forms were withdrawn in round 4.)
    CGSolve cg;
    CGMulti mm;  // KSPMatSolve's work vectors and per-column results (cg_multi.hip)
    int type = AIJHIP_KSP_CG;  // KSPType (aijhip_ksp_set_type); a change keeps the PC
    BCGSWork bw;               // BiCGStab's vectors beyond CG's (bcgs_solve.hip)
    aijhip_gamg_params_t gamg;
    aijhip_mg_smoother_t smoother;  // of every GAMG level but the coarsest (aijhip_ksp_set_mg_smoother)
    bool set_up = false;
    uint64_t a_gen = 0;  // the operator's plan generation at set-up: a re-planned
                         // operator (options, MatAssemblyEnd) is set up again
    uint64_t v_gen = 0;  // its values generation: new values (aijhip_mat_update_values)
                         // redo the PC set-up (D^-1, the GAMG hierarchy)
    double *d_hb = nullptr, *d_hx = nullptr;  // aijhip_ksp_solve_host's device copies of b and x
    std::vector<MGLevel> mg;                  // GAMG levels, finest first
    std::vector<aijhip::MGLevelView> mgview;  // what the V-cycle walks (mg_cycle.h)
    int32_t mat_vcycle = 0;     // columns the multi-column V-cycle is reserved for (0: KSPMatSolve refuses GAMG)
    aijhip::MGMultiBlocks mgm;  // its level blocks (aijhip_ksp_set_mat_vcycle_width)
    double *d_mgpart = nullptr;               // fused finest-level z.z / z.r partials
    double setup_seconds = 0.0;
    // how each level's coarsening was built (aijhip_ksp_get_gamg_setup_path)
    std::vector<int32_t> setup_path, setup_cols;
    bool setup_overflow = false;
    // -pc_gamg_reuse_interpolation (aijhip_ksp_set_gamg_reuse_interpolation):
    // new values on the structure the handle was set up on (s_gen: the
    // operator's structure generation then) refresh the hierarchy (gamg_refresh)
    bool reuse_interp = false;
    uint64_t s_gen = 0;
    int32_t n_full = 0, n_refreshed = 0;  // set-ups run (aijhip_ksp_get_gamg_setup_counts)
    // per level with a P: the pattern of A_l P_l (ai, aj; no values) kept
    // between refreshes, the row classes of it and of A_(l+1) (-1: not
    // counted yet), and whether the level's products go to the host builder
    // (a row past the numeric kernel's classes)
    std::vector<aijhip_gamg::DCsr> ap;
    std::vector<int> ap_cls, ac_cls;
    std::vector<char> host_level;
};

namespace {

void mg_free(aijhip_ksp *K) {
    for (MGLevel &L : K->mg) {
        if (L.own_A) aijhip_mat_destroy(L.A);
        aijhip_mat_destroy(L.P);
        hipFree(L.dinv); hipFree(L.b); hipFree(L.x); hipFree(L.r); hipFree(L.tdinv); hipFree(L.w);
    }
    K->mg.clear();
    K->mgview.clear();
    for (aijhip_gamg::DCsr &p : K->ap) p.release();
    K->ap.clear();
    K->ap_cls.clear();
    K->ac_cls.clear();
    K->host_level.clear();
    aijhip::mg_multi_free(K->mgm);
    hipFree(K->d_mgpart);
    K->d_mgpart = nullptr;
}

void ksp_free(aijhip_ksp *K) {
    mg_free(K);
    cg_free(K->cg);
    cgm_free(K->mm);
    bcgs_free(K->bw);
    hipFree(K->d_hb); hipFree(K->d_hx);
    K->d_hb = K->d_hx = nullptr;
    K->set_up = false;
}

}  // namespace

// x = B b: one V-cycle of K's hierarchy. dots != NULL: a fused finest
// post-smoothing leaves the z.z / z.b partials in d_mgpart (*dots, *nbz of
// each; *dots = NULL when that level is not fused).
int aijhip::ksp_pc_vcycle(aijhip_ksp *K, const double *b, double *x, hipStream_t s, const int *stop,
                          const double **dots, int *nbz) {
    bool done = false;
    const int rc = mg_vcycle(K->mgview, b, x, s, stop, dots ? K->d_mgpart : nullptr, &done);
    if (dots) {
        *dots = done ? K->d_mgpart : nullptr;
        *nbz = done ? K->mg[0].A->plan.n_blocks : 0;
    }
    return rc;
}

namespace {

// The multi-column V-cycle's level blocks and KSPMatSolve's work vectors for
// the reserved width, so that a solve allocates nothing
int reserve_mat_vcycle(aijhip_ksp *K) {
    if (K->mat_vcycle <= 0 || K->cg.pc != AIJHIP_PC_GAMG) return AIJHIP_OK;
    const int rc = aijhip::mg_multi_reserve(K->mgview, K->mat_vcycle, K->mgm);
    return rc ? rc : cgm_reserve(K->cg, K->mm, K->mat_vcycle);
}

// A diagonal PC on an m x k block of either layout: Z = D^-1 R (PCApply_Jacobi's
// product) or, dinv NULL, Z = R (PC none); one lane per entry
__global__ __launch_bounds__(kVecThreads) void k_pc_diag(int64_t m, int32_t k, int il, const double *__restrict__ dinv,
                                                         const double *R, int64_t ldr, double *Z, int64_t ldz) {
    GRID_STRIDE(t, m * k) {
        const int64_t i = il ? t / k : t % m, j = il ? t % k : t / m;
        const double r = R[il ? i * ldr + j : i + j * ldr];
        Z[il ? i * ldz + j : i + j * ldz] = dinv ? dinv[i] * r : r;
    }
}

// What the single-GPU handle plugs into the CG driver.
struct KspOperator final : CGOperator {
    aijhip_ksp *K;
    explicit KspOperator(aijhip_ksp *k) : K(k) { vcycle = k->cg.pc == AIJHIP_PC_GAMG; }
    int apply(const double *x, double *y, hipStream_t s, double *part, const CGState *S) override {
        const hipError_t e = part && K->cg.fused ? aijhip::launch_stream_dot(*K->A, x, y, part, &S->done, s)
                                                 : aijhip::launch_mult(*K->A, x, nullptr, y, false, s,
                                                                       part ? &S->done : nullptr);
        return e == hipSuccess ? AIJHIP_OK : cg_hip(e, "KSPSolve product");
    }
    int apply_stop(const double *x, double *y, hipStream_t s, const int *stop) override {
        const hipError_t e = aijhip::launch_mult(*K->A, x, nullptr, y, false, s, stop);
        return e == hipSuccess ? AIJHIP_OK : cg_hip(e, "KSPSolve product");
    }
    int pc_apply(const double *r, double *z, hipStream_t s, const int *stop, const double **dots,
                 int *nbz) override {
        return aijhip::ksp_pc_vcycle(K, r, z, s, stop, dots, nbz);
    }
    int wait(hipStream_t s) override {
        const hipError_t e = hipStreamSynchronize(s);
        return e == hipSuccess ? AIJHIP_OK : cg_hip(e, "KSPSolve poll");
    }
};

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
    int rc = aijhip::mg_check_smoother(K->smoother, &K->gamg);
    if (rc) return rc;
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
    rc = aijhip_gamg::build_device(A, K->gamg, dl, B, &more, &overflow, K->reuse_interp);
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
            return cg_hip(e, "GAMG: read level operator");
        }
        aijhip_gamg_params_t hp = K->gamg;
        hp.max_levels = K->gamg.max_levels - ((int32_t)dl.size() - 1);
        const int32_t nd_levels = (int32_t)dl.size();  // the host continues at level nd_levels - 1
        rc = aijhip_gamg::build_host_nns(L.m, ai.data(), aj.data(), aa.data(), B.data(), hp, &H, nd_levels - 1);
        if (rc) {
            aijhip_gamg::free_device_levels(dl);
            return cg_fail(rc, "GAMG: host hierarchy set-up failed");
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
    K->ap.assign((size_t)nl - 1, aijhip_gamg::DCsr());
    K->ap_cls.assign((size_t)nl - 1, -1);
    K->ac_cls.assign((size_t)nl - 1, -1);
    K->host_level.assign((size_t)nl - 1, 0);
    for (int32_t l = 0; l < nd; ++l) {  // (reuse-interpolation: the device levels' A P patterns)
        if (l + 1 < nl) K->ap[l] = dl[l].ap;
        else dl[l].ap.release();
        dl[l].ap = aijhip_gamg::DCsr();
    }
    std::vector<double> lambda((size_t)nl, 0.0);  // each level's emax(D^-1 A) estimate (none on the coarsest)
    for (int32_t hl = 0; hl + 1 < nh; ++hl)
        aijhip_gamg_host_level_info(H, hl, nullptr, nullptr, nullptr, &lambda[nd - 1 + hl]);
    for (int32_t l = 0; l < nd; ++l) {  // the device levels move into the KSP
        if (dl[l].P) lambda[l] = dl[l].emax;
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
            return cg_hip(e, "GAMG: level vectors");
        if (L.m > 0)
            hipLaunchKernelGGL(k_diag_inv, dim3((unsigned)((L.m + 255) / 256)), dim3(256), 0, nullptr, L.m,
                               L.A->d_ai, L.A->d_aj, L.A->d_aa, L.dinv);
        // the finest level on row templates: D^-1 per template for its fused
        // smoothing (pre-smoothing pass and post-smoothing epilogue read a
        // template id instead of D^-1; AIJHIP_KSP_EXPLICIT_Z=1 keeps dinv)
        if (l == 0 && L.m > 0 && L.A->plan.d_pid && L.A->plan.d_pval && !std::getenv("AIJHIP_KSP_EXPLICIT_Z")) {
            const int np = L.A->plan.n_pat;
            if ((e = hipMalloc(&L.tdinv, sizeof(double) * (size_t)np)) != hipSuccess)
                return cg_hip(e, "GAMG: template D^-1");
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
    for (int32_t l = 0; l + 1 < nl; ++l) {  // the smoother's scalars, and its third vector where it rotates one
        MGLevel &L = K->mg[l];
        if ((rc = aijhip::mg_set_smoother(K->smoother, lambda[l], L))) return rc;
        if (aijhip::mg_smoother_needs_w(L) &&
            (e = hipMalloc(&L.w, sizeof(double) * (size_t)std::max<int32_t>(L.m, 1))) != hipSuccess)
            return cg_hip(e, "GAMG: smoother vector");
    }
    if (K->mg[0].fused &&
        (e = hipMalloc(&K->d_mgpart, sizeof(double) * 2 * (size_t)std::max(1, K->mg[0].A->plan.n_blocks))) !=
            hipSuccess)
        return cg_hip(e, "GAMG partials");
    for (MGLevel &L : K->mg) {  // what the V-cycle walks
        L.Ad = L.A;
        L.Pd = L.P;
        K->mgview.push_back(L);
    }
    if ((e = hipDeviceSynchronize()) != hipSuccess) return cg_hip(e, "GAMG set-up");
    lap("level vectors, P^T");
    return AIJHIP_OK;
}

// A device CSR's arrays on the host (the refresh's host side)
struct HostCsr {
    std::vector<int32_t> ai, aj;
    std::vector<double> aa;
};
hipError_t read_back(const aijhip_mat &M, HostCsr &H, bool values = true) {
    H.ai.resize((size_t)M.m + 1);
    H.aj.resize((size_t)M.nz);
    H.aa.resize(values ? (size_t)M.nz : 0);
    hipError_t e = hipMemcpy(H.ai.data(), M.d_ai, sizeof(int32_t) * H.ai.size(), hipMemcpyDeviceToHost);
    if (e == hipSuccess && M.nz > 0)
        e = hipMemcpy(H.aj.data(), M.d_aj, sizeof(int32_t) * (size_t)M.nz, hipMemcpyDeviceToHost);
    if (e == hipSuccess && values && M.nz > 0)
        e = hipMemcpy(H.aa.data(), M.d_aa, sizeof(double) * (size_t)M.nz, hipMemcpyDeviceToHost);
    return e;
}

// A_(l+1)'s values by the host builder (a row past the numeric kernel's
// classes: how the set-up sends such a level to the host), on operands read
// back from the level handles, into the A_(l+1) handle's values
int galerkin_refresh_host(aijhip_ksp *K, int32_t l) {
    const aijhip_mat &Al = *K->mg[l].A, &Pl = *K->mg[l].P;
    aijhip_mat &Ac = *K->mg[l + 1].A;
    HostCsr a, p, c0;
    hipError_t e;
    if ((e = read_back(Al, a)) != hipSuccess || (e = read_back(Pl, p)) != hipSuccess ||
        (e = read_back(Ac, c0, false)) != hipSuccess)
        return cg_hip(e, "GAMG refresh: read level operands");
    std::vector<int32_t> ci, cj;
    std::vector<double> ca;
    const int rc = aijhip_gamg::galerkin_host(Al.m, a.ai.data(), a.aj.data(), a.aa.data(), Pl.n, p.ai.data(),
                                              p.aj.data(), p.aa.data(), K->gamg.threads, ci, cj, ca);
    if (rc) return cg_fail(rc, "GAMG refresh: host Galerkin product failed");
    if (ci != c0.ai || cj != c0.aj)
        return cg_fail(AIJHIP_ERR_STATE, "GAMG refresh: the level operator's pattern is not the product's");
    if (Ac.nz > 0 &&
        (e = hipMemcpy(Ac.d_aa, ca.data(), sizeof(double) * (size_t)Ac.nz, hipMemcpyHostToDevice)) != hipSuccess)
        return cg_hip(e, "GAMG refresh: level values");
    return AIJHIP_OK;
}

// PCSetUp_GAMG with -pc_gamg_reuse_interpolation on new values of the same
// structure (include/aijhip_ksp.h): every P_l, P_l^T and level pattern stays;
// A_(l+1) = P_l^T (A_l P_l) goes into the existing level operators by the
// numeric-only product (gamg_device.hip k_rowprod_numeric), then D^-1, the
// fused-launch choices and the smoothers follow the new values.
// AIJHIP_GAMG_LOG=1 prints the phases.
int gamg_refresh(aijhip_ksp *K) {
    aijhip::Range range("PCSetUp_GAMG (reuse interpolation)");
    const bool log = std::getenv("AIJHIP_GAMG_LOG") != nullptr;
    auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char *what, int32_t l) {
        if (!log) return;
        (void)hipDeviceSynchronize();
        const auto t = std::chrono::steady_clock::now();
        std::fprintf(stderr, "gamg refresh level %d %-18s %8.3f ms\n", l, what,
                     std::chrono::duration<double, std::milli>(t - t0).count());
        t0 = t;
    };
    const int32_t nl = (int32_t)K->mg.size();
    const int n_cu = std::max(K->A->n_cu, 1);
    int rc = AIJHIP_OK;
    hipError_t e = hipSuccess;
    // AIJHIP_GAMG_REFRESH=host sends every level's products to the host
    // builder (the path of a row past the numeric classes; the same bits)
    const char *side = std::getenv("AIJHIP_GAMG_REFRESH");
    const bool all_host = side && std::string(side) == "host";
    for (int32_t l = 0; l + 1 < nl; ++l) {
        MGLevel &L = K->mg[l];
        aijhip_mat &Ac = *K->mg[l + 1].A;
        if (all_host) K->host_level[l] = 1;
        if (!L.P->transpose && (rc = aijhip_mat_mult_transpose(L.P, L.r, K->mg[l + 1].b, nullptr))) return rc;
        const aijhip_gamg::DCsr Av = aijhip_gamg::csr_view(*L.A), Pv = aijhip_gamg::csr_view(*L.P),
                                PTv = aijhip_gamg::csr_view(*L.P->transpose);
        aijhip_gamg::DCsr &AP = K->ap[l];
        bool host = K->host_level[l] != 0;
        double *apv = nullptr;  // A P's values: transient
        if (!host && !AP.ai) {
            // no pattern yet (the flag was set after the set-up, or the host
            // built the level): the symbolic product once, its values as they come
            aijhip_gamg::DCsr T;
            rc = aijhip_gamg::rowprod_device(Av, Pv, T, n_cu, nullptr);
            if (rc == AIJHIP_ERR_STATE) host = true;
            else if (rc) return rc;
            else {
                apv = T.aa;
                T.aa = nullptr;
                AP = T;
            }
            lap("A*P (symbolic)", l);
        } else if (!host) {
            if ((e = aijhip_gamg::dalloc(&apv, AP.nz + 2)) != hipSuccess) return cg_hip(e, "GAMG refresh: A P values");
            rc = aijhip_gamg::rowprod_numeric_device(Av, Pv, AP.ai, AP.aj, apv, n_cu, &K->ap_cls[l]);
            if (rc == AIJHIP_ERR_STATE) host = true;
            else if (rc) {
                hipFree(apv);
                return rc;
            }
            lap("A*P (numeric)", l);
        }
        if (!host) {
            aijhip_gamg::DCsr APv = AP;
            APv.aa = apv;
            rc = aijhip_gamg::rowprod_numeric_device(PTv, APv, Ac.d_ai, Ac.d_aj, Ac.d_aa, n_cu, &K->ac_cls[l]);
            if (rc == AIJHIP_ERR_STATE) host = true;
            else if (rc) {
                hipFree(apv);
                return rc;
            }
            lap("P^T*(AP) (numeric)", l);
        }
        if ((e = hipDeviceSynchronize()) != hipSuccess) {
            hipFree(apv);
            return cg_hip(e, "GAMG refresh: Galerkin product");
        }
        hipFree(apv);
        if (host) {
            K->host_level[l] = 1;
            if ((rc = galerkin_refresh_host(K, l))) return rc;
            lap("host Galerkin", l);
        }
        // the level handle's value copies and codes follow its new values
        if ((rc = aijhip::values_changed(&Ac))) return rc;
        lap("level handle", l);
    }
    for (int32_t l = 0; l < nl; ++l) {
        MGLevel &L = K->mg[l];
        if (L.m > 0)
            hipLaunchKernelGGL(k_diag_inv, dim3((unsigned)((L.m + 255) / 256)), dim3(256), 0, nullptr, L.m,
                               L.A->d_ai, L.A->d_aj, L.A->d_aa, L.dinv);
        if (l == 0) {  // the finest plan may have gained or lost its templates
            hipFree(L.tdinv);
            L.tdinv = nullptr;
            if (L.m > 0 && L.A->plan.d_pid && L.A->plan.d_pval && !std::getenv("AIJHIP_KSP_EXPLICIT_Z")) {
                const int np = L.A->plan.n_pat;
                if ((e = hipMalloc(&L.tdinv, sizeof(double) * (size_t)np)) != hipSuccess)
                    return cg_hip(e, "GAMG: template D^-1");
                hipLaunchKernelGGL(k_tmpl_dinv, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, nullptr, np,
                                   L.A->plan.d_ptab, L.A->plan.d_pval, L.tdinv);
            }
        }
        L.nnz = L.A->nz;
        L.fused = !std::getenv("AIJHIP_MG_UNFUSED") && aijhip::stream_mg_fusable(*L.A);
    }
    if ((e = hipGetLastError()) != hipSuccess) return cg_hip(e, "GAMG refresh: D^-1");
    lap("D^-1", -1);
    for (int32_t l = 0; l + 1 < nl; ++l) {
        MGLevel &L = K->mg[l];
        double lambda = 0.0;
        if (K->smoother.type == AIJHIP_MG_SMOOTH_CHEBYSHEV) {
            // emax(D^-1 A_l) again, by the set-up's estimator: on the device
            // where the level's plan serves it, else the host builder's
            if (aijhip::stream_mg_fusable(*L.A)) {
                if ((rc = aijhip_gamg::emax_device(*L.A, L.dinv, K->gamg.eig_its, K->gamg.eig_ksp == 1, &lambda)))
                    return rc;
            } else {
                HostCsr a;
                if ((e = read_back(*L.A, a)) != hipSuccess) return cg_hip(e, "GAMG refresh: read level operator");
                lambda = aijhip_gamg::emax_host(L.m, a.ai.data(), a.aj.data(), a.aa.data(), K->gamg.eig_its,
                                                K->gamg.eig_ksp, K->gamg.threads);
            }
        }
        if ((rc = aijhip::mg_set_smoother(K->smoother, lambda, L))) return rc;
        if (aijhip::mg_smoother_needs_w(L) && !L.w &&
            (e = hipMalloc(&L.w, sizeof(double) * (size_t)std::max<int32_t>(L.m, 1))) != hipSuccess)
            return cg_hip(e, "GAMG: smoother vector");
    }
    lap("smoothers", -1);
    hipFree(K->d_mgpart);  // (the finest plan's blocks may have moved)
    K->d_mgpart = nullptr;
    if (K->mg[0].fused &&
        (e = hipMalloc(&K->d_mgpart, sizeof(double) * 2 * (size_t)std::max(1, K->mg[0].A->plan.n_blocks))) !=
            hipSuccess)
        return cg_hip(e, "GAMG partials");
    K->mgview.clear();
    for (MGLevel &L : K->mg) {
        L.Ad = L.A;
        L.Pd = L.P;
        K->mgview.push_back(L);
    }
    if ((e = hipDeviceSynchronize()) != hipSuccess) return cg_hip(e, "GAMG refresh");
    return AIJHIP_OK;
}

}  // namespace

extern "C" {

int aijhip_ksp_create(aijhip_mat_t A, aijhip_ksp_t *out) {
    if (!out) return cg_fail(AIJHIP_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!A) return cg_fail(AIJHIP_ERR_ARG, "NULL matrix");
    if (A->m != A->n) return cg_fail(AIJHIP_ERR_ARG, "KSP needs a square operator");
    aijhip_ksp *K = new (std::nothrow) aijhip_ksp();
    if (!K) return cg_fail(AIJHIP_ERR_ALLOC, "host allocation");
    K->A = A;
    aijhip_gamg_params_default(&K->gamg);
    aijhip_mg_smoother_default(&K->smoother);
    *out = K;
    return AIJHIP_OK;
}

int aijhip_ksp_set_tolerances(aijhip_ksp_t K, double rtol, double abstol, double dtol, int32_t max_it) {
    if (!K) return cg_fail(AIJHIP_ERR_ARG, "NULL ksp");
    DeviceGuard g(K->A->device);
    const int rc = cg_set_tolerances(K->cg, K->set_up, rtol, abstol, dtol, max_it);
    if (rc == AIJHIP_ERR_ALLOC) K->set_up = false;
    return rc;
}

int aijhip_ksp_set_pc_type(aijhip_ksp_t K, int pc) {
    if (!K) return cg_fail(AIJHIP_ERR_ARG, "NULL ksp");
    if (pc != AIJHIP_PC_NONE && pc != AIJHIP_PC_JACOBI && pc != AIJHIP_PC_GAMG)
        return cg_fail(AIJHIP_ERR_ARG, "unknown PC type");
    if (pc != K->cg.pc) K->set_up = false;
    K->cg.pc = pc;
    if (pc == AIJHIP_PC_GAMG)  // the set-up's streams, made once per process
        for (int slot = 0; slot < 2; ++slot) (void)aijhip_gamg::setup_stream(K->A->device, slot);
    return AIJHIP_OK;
}

int aijhip_ksp_set_type(aijhip_ksp_t K, int type) {
    if (!K) return cg_fail(AIJHIP_ERR_ARG, "NULL ksp");
    if (type != AIJHIP_KSP_CG && type != AIJHIP_KSP_BCGS)
        return cg_fail(AIJHIP_ERR_ARG, "unknown KSP type " + std::to_string(type) + " (AIJHIP_KSP_CG, AIJHIP_KSP_BCGS)");
    K->type = type;  // the PC and its set-up stay; BiCGStab's vectors come with the next set_up or solve
    return AIJHIP_OK;
}

int aijhip_ksp_get_type(aijhip_ksp_t K, int *type) {
    if (!K || !type) return cg_fail(AIJHIP_ERR_ARG, "NULL argument");
    *type = K->type;
    return AIJHIP_OK;
}

int aijhip_ksp_set_gamg_params(aijhip_ksp_t K, const aijhip_gamg_params_t *p) {
    if (!K) return cg_fail(AIJHIP_ERR_ARG, "NULL ksp");
    if (p) K->gamg = *p;
    else aijhip_gamg_params_default(&K->gamg);
    if (K->cg.pc == AIJHIP_PC_GAMG) K->set_up = false;
    return AIJHIP_OK;
}

int aijhip_ksp_set_mg_smoother(aijhip_ksp_t K, const aijhip_mg_smoother_t *sm) {
    if (!K) return cg_fail(AIJHIP_ERR_ARG, "NULL ksp");
    aijhip_mg_smoother_t v;
    aijhip_mg_smoother_default(&v);
    if (sm) v = *sm;
    const int rc = aijhip::mg_check_smoother(v);
    if (rc) return rc;
    K->smoother = v;
    if (K->cg.pc == AIJHIP_PC_GAMG) K->set_up = false;
    return AIJHIP_OK;
}

int aijhip_ksp_get_mg_smoother(aijhip_ksp_t K, int32_t l, int32_t *type, int32_t *its, double *emin, double *emax) {
    if (!K) return cg_fail(AIJHIP_ERR_ARG, "NULL ksp");
    if (!K->set_up || K->cg.pc != AIJHIP_PC_GAMG) return cg_fail(AIJHIP_ERR_STATE, "GAMG not set up");
    if (l < 0 || l + 1 >= (int32_t)K->mg.size())
        return cg_fail(AIJHIP_ERR_ARG, "no such smoothed level (the coarsest is preonly + Jacobi)");
    const MGLevel &L = K->mg[l];
    if (type) *type = L.smooth;
    if (its) *its = L.its;
    if (emin) *emin = L.cmin;
    if (emax) *emax = L.cmax;
    return AIJHIP_OK;
}

int aijhip_ksp_set_norm_type(aijhip_ksp_t K, int nt) {
    if (!K) return cg_fail(AIJHIP_ERR_ARG, "NULL ksp");
    if (nt < AIJHIP_KSP_NORM_NONE || nt > AIJHIP_KSP_NORM_NATURAL) return cg_fail(AIJHIP_ERR_ARG, "bad norm type");
    K->cg.normtype = nt;
    return AIJHIP_OK;
}

int aijhip_ksp_set_initial_guess_nonzero(aijhip_ksp_t K, int flg) {
    if (!K) return cg_fail(AIJHIP_ERR_ARG, "NULL ksp");
    K->cg.guess_nonzero = flg != 0;
    return AIJHIP_OK;
}

int aijhip_ksp_set_up(aijhip_ksp_t K) {
    aijhip::Range range("KSPSetUp");
    if (!K) return cg_fail(AIJHIP_ERR_ARG, "NULL ksp");
    if (K->set_up && K->a_gen == K->A->plan_gen && K->v_gen == K->A->values_gen) {
        if (K->type != AIJHIP_KSP_BCGS) return AIJHIP_OK;
        DeviceGuard g(K->A->device);  // a type set after the set-up: its vectors now, the PC as it is
        return bcgs_reserve(K->bw, K->A->m);
    }
    const auto t0 = std::chrono::steady_clock::now();
    aijhip_mat *A = K->A;
    DeviceGuard g(A->device);
    // reuse-interpolation: a set-up GAMG handle whose operator kept its
    // structure refreshes (CG's vectors and D^-1 follow the new plan and
    // values; the hierarchy's interpolations, patterns and blocks stay)
    const bool refresh = K->reuse_interp && K->set_up && K->cg.pc == AIJHIP_PC_GAMG && !K->mg.empty() &&
                         K->s_gen == A->struct_gen;
    int rc;
    if (refresh) {
        rc = cg_set_up(K->cg, *A, true);
        if (!rc) rc = gamg_refresh(K);
    } else {
        ksp_free(K);
        rc = cg_set_up(K->cg, *A, true);
        if (!rc && K->cg.pc == AIJHIP_PC_GAMG) rc = gamg_setup(K);
    }
    if (!rc) rc = reserve_mat_vcycle(K);
    if (!rc && K->type == AIJHIP_KSP_BCGS) rc = bcgs_reserve(K->bw, A->m);
    if (rc) {
        ksp_free(K);
        return rc;
    }
    K->setup_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    ++(refresh ? K->n_refreshed : K->n_full);
    K->set_up = true;
    K->a_gen = A->plan_gen;
    K->v_gen = A->values_gen;
    K->s_gen = A->struct_gen;
    return AIJHIP_OK;
}

int aijhip_ksp_set_gamg_reuse_interpolation(aijhip_ksp_t K, int flg) {
    if (!K) return cg_fail(AIJHIP_ERR_ARG, "NULL ksp");
    K->reuse_interp = flg != 0;
    return AIJHIP_OK;
}

int aijhip_ksp_get_gamg_reuse_interpolation(aijhip_ksp_t K, int *flg) {
    if (!K || !flg) return cg_fail(AIJHIP_ERR_ARG, "NULL argument");
    *flg = K->reuse_interp ? 1 : 0;
    return AIJHIP_OK;
}

int aijhip_ksp_get_mat_vcycle_reserve(aijhip_ksp_t K, int32_t cap, uint64_t *ptrs, int32_t *n) {
    if (!K || !n || (cap > 0 && !ptrs)) return cg_fail(AIJHIP_ERR_ARG, "NULL argument");
    std::vector<uint64_t> all;
    for (const aijhip::MGMultiBlocks::Level &L : K->mgm.lev)
        for (const double *p : {L.b, L.x, L.r, L.w}) all.push_back((uint64_t)reinterpret_cast<uintptr_t>(p));
    for (const double *p : {K->mm.d_r, K->mm.d_z, K->mm.d_p}) all.push_back((uint64_t)reinterpret_cast<uintptr_t>(p));
    for (int32_t q = 0; q < std::min<int32_t>(cap, (int32_t)all.size()); ++q) ptrs[q] = all[(size_t)q];
    *n = (int32_t)all.size();
    return AIJHIP_OK;
}

int aijhip_ksp_get_gamg_setup_counts(aijhip_ksp_t K, int32_t *full, int32_t *refreshed, double *last_seconds) {
    if (!K) return cg_fail(AIJHIP_ERR_ARG, "NULL ksp");
    if (full) *full = K->n_full;
    if (refreshed) *refreshed = K->n_refreshed;
    if (last_seconds) *last_seconds = K->setup_seconds;
    return AIJHIP_OK;
}

int aijhip_ksp_solve(aijhip_ksp_t K, const double *b, double *x, void *stream) {
    aijhip::Range range("KSPSolve");
    if (!K) return cg_fail(AIJHIP_ERR_ARG, "NULL ksp");
    if (K->type == AIJHIP_KSP_BCGS && K->cg.normtype != AIJHIP_KSP_NORM_PRECONDITIONED)
        return cg_fail(AIJHIP_ERR_STATE,
                       "BiCGStab serves the preconditioned norm only: it preconditions from the left, and the "
                       "other norm types need right preconditioning (aijhip_ksp_set_norm_type)");
    const int rc = aijhip_ksp_set_up(K);
    if (rc) return rc;
    DeviceGuard g(K->A->device);
    // iterations between polls: 8 (AIJHIP_KSP_POLL overrides it, for A/B)
    K->cg.poll = 8;
    if (const char *v = std::getenv("AIJHIP_KSP_POLL")) K->cg.poll = std::max(1, std::atoi(v));
    KspOperator op(K);
    if (K->type == AIJHIP_KSP_BCGS)
        return bcgs_solve(K->cg, K->bw, op, b, x, reinterpret_cast<hipStream_t>(stream));
    return cg_solve(K->cg, op, b, x, reinterpret_cast<hipStream_t>(stream));
}

int aijhip_ksp_get_iteration_number(aijhip_ksp_t K, int32_t *its) {
    if (!K || !its) return cg_fail(AIJHIP_ERR_ARG, "NULL argument");
    *its = K->cg.its;
    return AIJHIP_OK;
}

int aijhip_ksp_get_residual_norm(aijhip_ksp_t K, double *rnorm) {
    if (!K || !rnorm) return cg_fail(AIJHIP_ERR_ARG, "NULL argument");
    *rnorm = K->cg.rnorm;
    return AIJHIP_OK;
}

int aijhip_ksp_get_converged_reason(aijhip_ksp_t K, int *reason) {
    if (!K || !reason) return cg_fail(AIJHIP_ERR_ARG, "NULL argument");
    *reason = K->cg.reason;
    return AIJHIP_OK;
}

int aijhip_ksp_get_residual_history(aijhip_ksp_t K, double *hist, int32_t na, int32_t *n) {
    if (!K || !n || (na > 0 && !hist)) return cg_fail(AIJHIP_ERR_ARG, "NULL argument");
    const int32_t c = std::min<int32_t>(na, (int32_t)K->cg.hist.size());
    std::copy(K->cg.hist.begin(), K->cg.hist.begin() + c, hist);
    *n = c;
    return AIJHIP_OK;
}

int aijhip_ksp_get_host_syncs(aijhip_ksp_t K, int32_t *n) {
    if (!K || !n) return cg_fail(AIJHIP_ERR_ARG, "NULL argument");
    *n = K->cg.waits;
    return AIJHIP_OK;
}

int aijhip_ksp_get_iteration_bytes(aijhip_ksp_t K, int64_t *bytes, int64_t *spmv_bytes, int64_t *level0) {
    if (!K || !bytes) return cg_fail(AIJHIP_ERR_ARG, "NULL argument");
    if (!K->set_up) return cg_fail(AIJHIP_ERR_STATE, "KSP is not set up");
    const int64_t m = K->A->m;
    const int64_t a0 = aijhip::mult_layout_bytes(*K->A);
    // CG: p = z + b p with x += a p (reads z, p, x; writes p, x), the SpMV
    // (p . w in its epilogue), the r update (Jacobi: reads r, w, D^-1,
    // writes r, z; GAMG: reads r, w, writes r; z from the V-cycle)
    // (Jacobi on row templates, Z not stored: p = z + b p reads r and a
    // template id instead of z; the update reads r, w and an id, writes r)
    int64_t spmv = a0, vec = K->cg.implicit_z ? 41 * m + 25 * m : 40 * m + (K->cg.pc == AIJHIP_PC_GAMG ? 24 * m : 40 * m);
    if (!K->cg.fused) vec += 16 * m;  // p . w in its own pass
    // BiCGStab: two products, two PC applications (nk) and its five vector
    // passes: p = r - (omegaold beta) v + beta p 32 m; v = D^-1 v with v.rp
    // 32 m (none / GAMG: 16 m, v and rp read only); s = r - alpha v 24 m;
    // t = D^-1 t with s.t, t.t, s.s 32 m (none / GAMG: 16 m); the x / r
    // update with r.r, r.rp 56 m (reads x, p, s, t, rp; writes x, r)
    const bool bcgs = K->type == AIJHIP_KSP_BCGS;
    const int64_t nk = bcgs ? 2 : 1;
    if (bcgs) {
        spmv = 2 * a0;
        vec = (K->cg.pc == AIJHIP_PC_JACOBI ? 176 : 144) * m;
    }
    int64_t lev0 = spmv + vec;
    if (K->cg.pc == AIJHIP_PC_GAMG) {
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
                // another smoother's added products and their row operands
                // (include/aijhip_ksp.h lists them; D: D^-1 or a template id)
                const int64_t k = L.its, D = L.fused && L.tdinv ? 1 : 8;
                if (L.smooth == AIJHIP_MG_SMOOTH_CHEBYSHEV) {
                    sp += 2 * k * la;
                    v += L.fused ? ((8 + D) + (k - 1) * (16 + D) + k * (16 + D)) * ml
                                 : (40 + (k - 1) * 48 + k * 48) * ml;
                } else {
                    sp += 2 * (k - 1) * la;
                    v += 2 * (k - 1) * (L.fused ? 8 + D : 40) * ml;
                }
            }
            spmv += nk * sp;
            vec += nk * v;
            if (l == 0) lev0 += nk * (sp + v);
        }
    }
    *bytes = spmv + vec;
    if (spmv_bytes) *spmv_bytes = spmv;
    if (level0) *level0 = lev0;
    return AIJHIP_OK;
}

int aijhip_ksp_get_fused(aijhip_ksp_t K, int *fused) {
    if (!K || !fused) return cg_fail(AIJHIP_ERR_ARG, "NULL argument");
    *fused = K->type == AIJHIP_KSP_CG && K->cg.fused ? 1 : 0;
    return AIJHIP_OK;
}

int aijhip_ksp_get_pc_levels(aijhip_ksp_t K, int32_t *nlevels, int32_t *rows, int64_t *nnz, int32_t cap,
                             double *setup_seconds) {
    if (!K || !nlevels) return cg_fail(AIJHIP_ERR_ARG, "NULL argument");
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
        return cg_fail(AIJHIP_ERR_ARG, "no such PC level (set up a GAMG KSP first)");
    const aijhip_mat *M = which == 'A' ? K->mg[l].A : K->mg[l].P;
    if (!M) return cg_fail(AIJHIP_ERR_ARG, "the coarsest level has no interpolation");
    if (m) *m = M->m;
    if (n) *n = M->n;
    if (nnz) *nnz = M->nz;
    if (!ai) return AIJHIP_OK;
    DeviceGuard g(M->device);
    hipError_t e = hipMemcpy(ai, M->d_ai, sizeof(int32_t) * ((size_t)M->m + 1), hipMemcpyDeviceToHost);
    if (e == hipSuccess && aj && M->nz > 0) e = hipMemcpy(aj, M->d_aj, sizeof(int32_t) * (size_t)M->nz, hipMemcpyDeviceToHost);
    if (e == hipSuccess && aa && M->nz > 0) e = hipMemcpy(aa, M->d_aa, sizeof(double) * (size_t)M->nz, hipMemcpyDeviceToHost);
    return e == hipSuccess ? AIJHIP_OK : cg_hip(e, "read PC level");
}

int aijhip_ksp_get_gamg_setup_path(aijhip_ksp_t K, int32_t cap, int32_t *path, int32_t *product_cols,
                                   int32_t *host_fallback) {
    if (!K) return cg_fail(AIJHIP_ERR_ARG, "null ksp");
    if (!K->set_up || K->cg.pc != AIJHIP_PC_GAMG) return cg_fail(AIJHIP_ERR_STATE, "GAMG not set up");
    const size_t n = std::min<size_t>(K->setup_path.size(), (size_t)std::max(cap, 0));
    for (size_t l = 0; l < n; ++l) {
        if (path) path[l] = K->setup_path[l];
        if (product_cols) product_cols[l] = K->setup_cols[l];
    }
    if (host_fallback) *host_fallback = K->setup_overflow ? 1 : 0;
    return AIJHIP_OK;
}

int aijhip_ksp_solve_host(aijhip_ksp_t K, const double *b, double *x) {
    if (!K) return cg_fail(AIJHIP_ERR_ARG, "NULL ksp");
    const int64_t m = K->A->m;
    if (m > 0 && (!b || !x)) return cg_fail(AIJHIP_ERR_ARG, "NULL vector");
    if (b == x) return cg_fail(AIJHIP_ERR_ARG, "b and x alias");
    int rc = aijhip_ksp_set_up(K);
    if (rc) return rc;
    DeviceGuard g(K->A->device);
    hipError_t e = hipSuccess;
    if (!K->d_hb && (e = hipMalloc(&K->d_hb, sizeof(double) * (size_t)std::max<int64_t>(m, 1))) != hipSuccess)
        return cg_hip(e, "KSPSolve host vectors");
    if (!K->d_hx && (e = hipMalloc(&K->d_hx, sizeof(double) * (size_t)std::max<int64_t>(m, 1))) != hipSuccess)
        return cg_hip(e, "KSPSolve host vectors");
    // b (and a nonzero initial guess) up once, x down once: 2 x 8m bytes over
    // PCIe per solve instead of per MatMult (the reference's step-2 copies)
    if (m > 0 && ((e = hipMemcpy(K->d_hb, b, sizeof(double) * (size_t)m, hipMemcpyHostToDevice)) != hipSuccess ||
                  (K->cg.guess_nonzero &&
                   (e = hipMemcpy(K->d_hx, x, sizeof(double) * (size_t)m, hipMemcpyHostToDevice)) != hipSuccess)))
        return cg_hip(e, "KSPSolve b / x in");
    if ((rc = aijhip_ksp_solve(K, K->d_hb, K->d_hx, nullptr))) return rc;
    if (m > 0 && (e = hipMemcpy(x, K->d_hx, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost)) != hipSuccess)
        return cg_hip(e, "KSPSolve x out");
    return AIJHIP_OK;
}

}  // extern "C"

namespace {

// Whether an element of the m x k block at B is an element of the one at X.
// A block is `cnt` runs of `run` doubles, ld apart (interleaved: m rows of k;
// columns: k columns of m). With one leading dimension the test is exact, so
// two column ranges of one wider array are distinct blocks; otherwise the
// blocks' address ranges are compared.
bool blocks_overlap(bool il, int64_t m, int64_t k, const double *B, int64_t ldb, const double *X, int64_t ldx) {
    const int64_t run = il ? k : m, cnt = il ? m : k;
    if (run <= 0 || cnt <= 0 || !B || !X) return false;
    const intptr_t db = reinterpret_cast<intptr_t>(X) - reinterpret_cast<intptr_t>(B);
    if (ldb == ldx && db % (intptr_t)sizeof(double) == 0) {
        // B(i, j) = i ld + j and X(i', j') = d + i' ld + j' coincide iff
        // (i - i') ld = d + t with t = j' - j in (-run, run)
        const int64_t ld = ldb, d = (int64_t)(db / (intptr_t)sizeof(double));
        const int64_t r = ((-d) % ld + ld) % ld;
        const int64_t cand[2] = {r, r - ld};
        for (const int64_t t : cand) {
            if (t <= -run || t >= run) continue;
            const int64_t q = (d + t) / ld;
            if (q > -cnt && q < cnt) return true;
        }
        return false;
    }
    const uintptr_t b0 = reinterpret_cast<uintptr_t>(B), x0 = reinterpret_cast<uintptr_t>(X);
    const uintptr_t be = b0 + sizeof(double) * (size_t)((cnt - 1) * ldb + run);
    const uintptr_t xe = x0 + sizeof(double) * (size_t)((cnt - 1) * ldx + run);
    return b0 < xe && x0 < be;
}

const char *const kNoWidth =
    "KSPMatSolve serves PC none and Jacobi: the V-cycle has no multi-column "
    "form (solve the columns one by one with aijhip_ksp_solve)";

const char *const kNoBcgsMat =
    "KSPMatSolve's lock-step solver is CG: a BiCGStab handle (AIJHIP_KSP_BCGS) solves the columns one by one "
    "with aijhip_ksp_solve";

// Whether the handle's PC has a multi-column form at width k: none and Jacobi
// always, GAMG within the reserved width (aijhip_ksp_set_mat_vcycle_width)
int mat_width_check(aijhip_ksp_t K, int32_t k) {
    if (K->cg.pc == AIJHIP_PC_NONE || K->cg.pc == AIJHIP_PC_JACOBI) return AIJHIP_OK;
    if (K->cg.pc != AIJHIP_PC_GAMG || K->mat_vcycle == 0) return cg_fail(AIJHIP_ERR_STATE, kNoWidth);
    if (k > K->mat_vcycle)
        return cg_fail(AIJHIP_ERR_STATE, "k = " + std::to_string(k) + " is above the reserved V-cycle width " +
                                             std::to_string(K->mat_vcycle) + " (aijhip_ksp_set_mat_vcycle_width)");
    return AIJHIP_OK;
}

// KSPMatSolve's argument checks, all before any device work. *go = 0: nothing to do (k = 0).
int mat_solve_check(aijhip_ksp_t K, int32_t k, int layout, const double *B, int64_t ldb, const double *X, int64_t ldx,
                    int *go) {
    *go = 0;
    if (!K) return cg_fail(AIJHIP_ERR_ARG, "NULL ksp");
    if (k < 0 || k > AIJHIP_KSP_MAX_RHS)
        return cg_fail(AIJHIP_ERR_ARG, "k = " + std::to_string(k) + " is outside 0.." + std::to_string(AIJHIP_KSP_MAX_RHS));
    if (layout != AIJHIP_DENSE_COLUMNS && layout != AIJHIP_DENSE_INTERLEAVED)
        return cg_fail(AIJHIP_ERR_ARG, "unknown dense layout " + std::to_string(layout));
    if (k == 0) return AIJHIP_OK;
    const bool il = layout == AIJHIP_DENSE_INTERLEAVED;
    const int64_t m = K->A->m, minld = il ? k : m;
    if (ldb < minld) return cg_fail(AIJHIP_ERR_ARG, "ldb " + std::to_string(ldb) + " is below " + std::to_string(minld));
    if (ldx < minld) return cg_fail(AIJHIP_ERR_ARG, "ldx " + std::to_string(ldx) + " is below " + std::to_string(minld));
    if (m > 0 && (!B || !X)) return cg_fail(AIJHIP_ERR_ARG, "NULL dense array");
    if (blocks_overlap(il, m, k, B, ldb, X, ldx)) return cg_fail(AIJHIP_ERR_ARG, "B and X overlap");
    if (const int rc = mat_width_check(K, k)) return rc;
    *go = 1;
    return AIJHIP_OK;
}

int32_t mat_solve_chunks(int32_t k) { return k / 8 + ((k & 4) != 0) + ((k & 2) != 0) + (k & 1); }

}  // namespace

extern "C" {

int aijhip_ksp_mat_solve(aijhip_ksp_t K, int32_t k, int layout, const double *B, int64_t ldb, double *X, int64_t ldx,
                         void *stream) {
    aijhip::Range range("KSPMatSolve");
    if (K && K->type == AIJHIP_KSP_BCGS) return cg_fail(AIJHIP_ERR_STATE, kNoBcgsMat);
    int go = 0;
    int rc = mat_solve_check(K, k, layout, B, ldb, X, ldx, &go);
    if (rc || !go) return rc;
    if ((rc = aijhip_ksp_set_up(K))) return rc;
    DeviceGuard g(K->A->device);
    K->cg.poll = 8;
    if (const char *v = std::getenv("AIJHIP_KSP_POLL")) K->cg.poll = std::max(1, std::atoi(v));
    const CGMultiPC mg{&K->mgview, &K->mgm};
    return cgm_solve(K->cg, K->mm, *K->A, k, layout, B, ldb, X, ldx, reinterpret_cast<hipStream_t>(stream),
                     K->cg.pc == AIJHIP_PC_GAMG ? &mg : nullptr);
}

int aijhip_ksp_set_mat_vcycle_width(aijhip_ksp_t K, int32_t kmax) {
    if (kmax < 0 || kmax > AIJHIP_KSP_MAX_RHS)
        return cg_fail(AIJHIP_ERR_ARG,
                       "kmax = " + std::to_string(kmax) + " is outside 0.." + std::to_string(AIJHIP_KSP_MAX_RHS));
    if (!K) return cg_fail(AIJHIP_ERR_ARG, "NULL ksp");
    K->mat_vcycle = kmax;
    if (!K->set_up || K->a_gen != K->A->plan_gen || K->v_gen != K->A->values_gen) return AIJHIP_OK;
    DeviceGuard g(K->A->device);  // a set-up handle: the blocks now, the hierarchy as it is
    return reserve_mat_vcycle(K);
}

int aijhip_ksp_get_mat_vcycle_width(aijhip_ksp_t K, int32_t *kmax) {
    if (!K || !kmax) return cg_fail(AIJHIP_ERR_ARG, "NULL argument");
    *kmax = K->mat_vcycle;
    return AIJHIP_OK;
}

int aijhip_ksp_pc_apply(aijhip_ksp_t K, const double *r, double *z, void *stream) {
    if (!K) return cg_fail(AIJHIP_ERR_ARG, "NULL ksp");
    const int64_t m = K->A->m;
    if (m > 0 && (!r || !z)) return cg_fail(AIJHIP_ERR_ARG, "NULL vector");
    if (m > 0 && r == z) return cg_fail(AIJHIP_ERR_ARG, "r and z alias");
    const int rc = aijhip_ksp_set_up(K);
    if (rc || m == 0) return rc;
    DeviceGuard g(K->A->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (K->cg.pc == AIJHIP_PC_GAMG) return aijhip::ksp_pc_vcycle(K, r, z, s, nullptr, nullptr, nullptr);
    hipLaunchKernelGGL(k_pc_diag, dim3(K->cg.vec_grid), dim3(kVecThreads), 0, s, m, 1, 1,
                       K->cg.pc == AIJHIP_PC_JACOBI ? K->cg.d_dinv : nullptr, r, (int64_t)1, z, (int64_t)1);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? AIJHIP_OK : cg_hip(e, "PCApply");
}

int aijhip_ksp_pc_mat_apply(aijhip_ksp_t K, int32_t k, int layout, const double *R, int64_t ldr, double *Z,
                            int64_t ldz, void *stream) {
    int go = 0;
    int rc = mat_solve_check(K, k, layout, R, ldr, Z, ldz, &go);
    if (rc || !go) return rc;
    if ((rc = aijhip_ksp_set_up(K))) return rc;
    const int64_t m = K->A->m;
    if (m == 0) return AIJHIP_OK;
    DeviceGuard g(K->A->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool il = layout == AIJHIP_DENSE_INTERLEAVED;
    if (K->cg.pc != AIJHIP_PC_GAMG) {
        const int64_t n = m * k;
        const dim3 grid((unsigned)std::max<int64_t>(
            1, std::min<int64_t>((n + kVecThreads - 1) / kVecThreads, (int64_t)K->A->n_cu * 8)));
        hipLaunchKernelGGL(k_pc_diag, grid, dim3(kVecThreads), 0, s, m, k, il ? 1 : 0,
                           K->cg.pc == AIJHIP_PC_JACOBI ? K->cg.d_dinv : nullptr, R, ldr, Z, ldz);
        const hipError_t e = hipGetLastError();
        return e == hipSuccess ? AIJHIP_OK : cg_hip(e, "PCMatApply");
    }
    // the V-cycle runs on tight interleaved blocks: others go through the
    // handle's finest staging blocks
    const double *rt = R;
    double *zt = Z;
    if (!il || ldr != k) {
        cgm_copy_block(m, k, K->A->n_cu, R, ldr, il, K->mgm.lev[0].b, k, true, s);
        rt = K->mgm.lev[0].b;
    }
    if (!il || ldz != k) zt = K->mgm.lev[0].x;
    if ((rc = aijhip::mg_vcycle_multi(K->mgview, K->mgm, k, rt, zt, s, nullptr))) return rc;
    if (zt != Z) cgm_copy_block(m, k, K->A->n_cu, zt, k, true, Z, ldz, il, s);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? AIJHIP_OK : cg_hip(e, "PCMatApply");
}

int aijhip_ksp_mat_solve_host(aijhip_ksp_t K, int32_t k, int layout, const double *B, int64_t ldb, double *X,
                              int64_t ldx) {
    if (K && K->type == AIJHIP_KSP_BCGS) return cg_fail(AIJHIP_ERR_STATE, kNoBcgsMat);
    int go = 0;
    int rc = mat_solve_check(K, k, layout, B, ldb, X, ldx, &go);
    if (rc || !go) return rc;
    if ((rc = aijhip_ksp_set_up(K))) return rc;
    const int64_t m = K->A->m;
    if (m == 0) return aijhip_ksp_mat_solve(K, k, layout, B, ldb, X, ldx, nullptr);
    DeviceGuard g(K->A->device);
    // tight device copies of the two blocks (runs of `run` doubles, the host
    // arrays' leading dimensions stripped by the 2-D copies): nothing of X
    // outside its m x k block is read or written
    const bool il = layout == AIJHIP_DENSE_INTERLEAVED;
    const size_t run = il ? (size_t)k : (size_t)m, cnt = il ? (size_t)m : (size_t)k;
    double *dB = nullptr, *dX = nullptr;
    hipError_t e = hipMalloc(&dB, sizeof(double) * run * cnt);
    if (e == hipSuccess) e = hipMalloc(&dX, sizeof(double) * run * cnt);
    if (e == hipSuccess)
        e = hipMemcpy2D(dB, sizeof(double) * run, B, sizeof(double) * (size_t)ldb, sizeof(double) * run, cnt,
                        hipMemcpyHostToDevice);
    if (e == hipSuccess && K->cg.guess_nonzero)
        e = hipMemcpy2D(dX, sizeof(double) * run, X, sizeof(double) * (size_t)ldx, sizeof(double) * run, cnt,
                        hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        rc = aijhip_ksp_mat_solve(K, k, layout, dB, (int64_t)run, dX, (int64_t)run, nullptr);
        if (!rc)
            e = hipMemcpy2D(X, sizeof(double) * (size_t)ldx, dX, sizeof(double) * run, sizeof(double) * run, cnt,
                            hipMemcpyDeviceToHost);
    }
    (void)hipFree(dB);
    (void)hipFree(dX);
    if (rc) return rc;
    return e == hipSuccess ? AIJHIP_OK : cg_hip(e, "KSPMatSolve with host arrays");
}

int aijhip_ksp_get_mat_solve_results(aijhip_ksp_t K, int32_t cap, int32_t *its, int *reason, double *rnorm,
                                     int32_t *k) {
    if (!K) return cg_fail(AIJHIP_ERR_ARG, "NULL ksp");
    const CGMulti &mm = K->mm;
    const int32_t n = std::min<int32_t>(std::max<int32_t>(cap, 0), mm.k);
    for (int32_t j = 0; j < n; ++j) {
        if (its) its[j] = mm.its[j];
        if (reason) reason[j] = mm.reason[j];
        if (rnorm) rnorm[j] = mm.rnorm[j];
    }
    if (k) *k = mm.k;
    return AIJHIP_OK;
}

int aijhip_ksp_get_mat_solve_history(aijhip_ksp_t K, int32_t column, double *hist, int32_t na, int32_t *n) {
    if (!K) return cg_fail(AIJHIP_ERR_ARG, "NULL ksp");
    if (!n || (na > 0 && !hist)) return cg_fail(AIJHIP_ERR_ARG, "NULL argument");
    if (column < 0 || column >= K->mm.k)
        return cg_fail(AIJHIP_ERR_ARG, "the last mat_solve has no column " + std::to_string(column));
    const std::vector<double> &h = K->mm.hist[column];
    const int32_t c = std::min<int32_t>(std::max<int32_t>(na, 0), (int32_t)h.size());
    std::copy(h.begin(), h.begin() + c, hist);
    *n = c;
    return AIJHIP_OK;
}

int aijhip_ksp_get_mat_solve_bytes(aijhip_ksp_t K, int32_t k, int64_t *bytes, int64_t *spmm_bytes) {
    if (!K) return cg_fail(AIJHIP_ERR_ARG, "NULL ksp");
    if (!bytes) return cg_fail(AIJHIP_ERR_ARG, "NULL argument");
    if (k < 0 || k > AIJHIP_KSP_MAX_RHS) return cg_fail(AIJHIP_ERR_ARG, "k is outside 0..AIJHIP_KSP_MAX_RHS");
    if (!K->set_up) return cg_fail(AIJHIP_ERR_STATE, "KSP is not set up");
    if (K->cg.pc != AIJHIP_PC_NONE && K->cg.pc != AIJHIP_PC_JACOBI && (K->cg.pc != AIJHIP_PC_GAMG || K->mat_vcycle == 0))
        return cg_fail(AIJHIP_ERR_STATE, "KSPMatSolve serves PC none and Jacobi: the V-cycle has no multi-column form");
    int rc = mat_width_check(K, k);
    if (rc) return rc;
    int64_t sp = 0;
    rc = aijhip_mat_mat_mult_get_plan(K->A, k, AIJHIP_DENSE_INTERLEAVED, nullptr, nullptr, &sp);
    if (rc) return rc;
    if (K->cg.pc == AIJHIP_PC_GAMG) {
        // CG: km_aypx 40 m k, km_dot 16 m k, km_update 24 m k (reads R, W;
        // writes R), km_dots 16 m k (reads Z, R). The V-cycle, per smoothed
        // level of m_l rows: every product at its MatMatMult bytes (A_l 2 its
        // times for Richardson(its), 2 its + 2 for Chebyshev(its), P and P^T
        // once), the start x = f D^-1 b 16 m_l k + 8 m_l (reads b, D^-1; writes
        // x), and the epilogues' row operands beyond a product's own X and Y:
        // residual 8 m_l k (b), interpolation 8 m_l k (x), a Richardson step
        // 8 m_l k + 8 m_l chunks (b, D^-1), a Chebyshev step with p_km1
        // 16 m_l k + 8 m_l chunks; the coarse solve 16 m_c k + 8 m_c.
        const int64_t m = K->A->m, ch = mat_solve_chunks(k);
        int64_t vec = 96 * m * k;
        const int nl = (int)K->mg.size();
        for (int l = 0; l < nl; ++l) {
            const MGLevel &L = K->mg[l];
            const int64_t ml = L.m;
            vec += 16 * ml * k + 8 * ml;
            if (l == nl - 1) break;
            const bool cheby = L.smooth == AIJHIP_MG_SMOOTH_CHEBYSHEV;
            const int64_t its = L.its;
            const int64_t n_rich = cheby ? 1 : 2 * its - 1;   // steps of the Richardson form (Chebyshev's start going up)
            const int64_t n_cheb = cheby ? 2 * its : 0;       // Chebyshev steps; the first going down has no p_km1
            const int64_t n_pm1 = cheby ? 2 * its - 1 : 0;
            int64_t la = 0, lp = 0, lt = 0;
            if ((rc = aijhip_mat_mat_mult_get_plan(L.A, k, AIJHIP_DENSE_INTERLEAVED, nullptr, nullptr, &la)) ||
                (rc = aijhip_mat_mat_mult_get_plan(L.P, k, AIJHIP_DENSE_INTERLEAVED, nullptr, nullptr, &lp)) ||
                (rc = aijhip_mat_mat_mult_get_plan(L.P->transpose, k, AIJHIP_DENSE_INTERLEAVED, nullptr, nullptr, &lt)))
                return rc;
            sp += (n_rich + n_cheb + 1) * la + lp + lt;
            vec += 8 * ml * k + 8 * ml * k + (n_rich + n_cheb) * (8 * ml * k + 8 * ml * ch) + n_pm1 * 8 * ml * k;
        }
        *bytes = sp + vec;
        if (spmm_bytes) *spmm_bytes = sp;
        return AIJHIP_OK;
    }
    // km_aypx 40 m k (reads Z, P, X; writes P, X), km_dot 16 m k (reads P, W),
    // km_update 32 m k (reads R, W; writes R, Z) and, Jacobi, D^-1 once per chunk
    const int64_t m = K->A->m;
    const int64_t vec = 88 * m * k + (K->cg.pc == AIJHIP_PC_JACOBI ? 8 * m * mat_solve_chunks(k) : 0);
    *bytes = sp + vec;
    if (spmm_bytes) *spmm_bytes = sp;
    return AIJHIP_OK;
}

int aijhip_ksp_destroy(aijhip_ksp_t K) {
    if (!K) return AIJHIP_OK;
    {
        DeviceGuard g(K->A->device);
        (void)hipDeviceSynchronize();
        ksp_free(K);
    }
    delete K;
    return AIJHIP_OK;
}

}  // extern "C"
