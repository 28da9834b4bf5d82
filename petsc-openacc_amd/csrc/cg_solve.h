// cg_solve.h — the one preconditioned-CG driver (cg_solve.hip) behind both
// solver handles: aijhip_ksp (ksp.hip, one GPU) and aijhip_kspmpi
// (ksp_mpi.hip, one process per GPU). Each handle holds a CGSolve and plugs
// what differs between the two into a CGOperator. Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "aijhip_internal.h"
#include "cg_device.h"

// Shared by the driver and both handles: the error returns and the device guard.
inline int cg_fail(int code, const std::string &msg) {
    aijhip::set_error(msg);
    return code;
}
inline int cg_hip(hipError_t e, const char *what) {
    return cg_fail(AIJHIP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur != dev && hipSetDevice(dev) == hipSuccess) prev = cur;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// The tolerances, CG's device vectors and the last solve's results.
struct CGSolve {
    double rtol = 1e-5, abstol = 1e-50, dtol = 1e5;
    int32_t max_it = 10000;
    int pc = AIJHIP_PC_JACOBI;
    int normtype = AIJHIP_KSP_NORM_PRECONDITIONED;
    bool guess_nonzero = false;
    int32_t poll = 8;  // iterations launched between two reads of the stop flag
    // the set-up (cg_set_up)
    int64_t m = 0;
    bool fused = false;  // p.w partials from the STREAM SpMV epilogue (else k_dot)
    int vec_grid = 1;    // blocks of the vector kernels = partials per quantity
    int n_dparts = 1;    // p.w partials of the diagonal block: STREAM blocks when fused, else vec_grid
    // CG + Jacobi on row templates: D^-1 per template (d_tdinv, indexed by
    // the operator's template ids pid) and Z not stored (k_aypx / k_update IZ)
    bool implicit_z = false;
    const uint8_t *pid = nullptr;
    double *d_dinv = nullptr, *d_tdinv = nullptr, *d_r = nullptr, *d_z = nullptr, *d_p = nullptr,
           *d_part = nullptr, *d_red = nullptr, *d_hist = nullptr;
    int32_t hist_cap = 0;
    CGState *d_state = nullptr;
    CGState *h_state = nullptr;  // pinned
    // the last solve (waits: the polls and the final read)
    int32_t its = 0, waits = 0;
    int reason = 0;
    double rnorm = 0.0;
    std::vector<double> hist;
};

struct CGRun;

// What differs between the two solvers, and nothing else.
struct CGOperator {
    bool multi = false;       // more than one rank: red[] is all-reduced before each scalar step
    bool vcycle = false;      // the PC is a V-cycle (pc_apply); Jacobi / none stay inside k_init / k_update
    double *opart = nullptr;  // the off-diagonal block's p.w correction partials (apply leaves nob of them)
    int nob = 0;
    virtual ~CGOperator() = default;
    // y = A x on s. part == NULL: the plain product. Else CG's W = A P: it
    // honours the stop flag S->done and, when the set-up is fused, leaves the
    // n_dparts p.w partials in part (and the A_o list in opart).
    virtual int apply(const double *x, double *y, hipStream_t s, double *part, const CGState *S) = 0;
    // the plain product under a device stop flag (BiCGStab's, bcgs_solve.hip):
    // y may be left unwritten once *stop is set. An operator whose product
    // takes no flag runs the plain product: nothing reads y after the stop.
    virtual int apply_stop(const double *x, double *y, hipStream_t s, const int * /*stop*/) {
        return apply(x, y, s, nullptr, nullptr);
    }
    // in-place sum of red[0, n) over the ranks (multi only)
    virtual int allreduce(double *, int, hipStream_t) { return AIJHIP_OK; }
    // z = B r, one V-cycle (vcycle only). dots != NULL: *dots = the z.z / z.r
    // partials of a fused finest post-smoothing (*nbz of each), or NULL.
    virtual int pc_apply(const double *r, double *z, hipStream_t s, const int *stop, const double **dots, int *nbz);
    // block the host until s has drained
    virtual int wait(hipStream_t s) = 0;
    // n iterations on s: plain launches (the distributed handle's HIP-graph
    // capture / replay wraps this)
    virtual int run_batch(const CGRun &R, int32_t n, hipStream_t s);
};

// One solve in flight: what cg_iteration launches from.
struct CGRun {
    CGSolve &cg;
    CGOperator &op;
    double *x;
    CGParams p;
};

// Allocate the vectors for the square block A (freeing a previous set-up) and
// form D^-1. implicit_z: Jacobi on row templates may leave Z unstored
// (AIJHIP_KSP_EXPLICIT_Z=1 keeps it, for A/B).
int cg_set_up(CGSolve &cg, const aijhip_mat &A, bool implicit_z);
void cg_free(CGSolve &cg);
// The tolerances; a set-up handle regrows its history only (AIJHIP_ERR_ALLOC:
// the handle must be set up again).
int cg_set_tolerances(CGSolve &cg, bool set_up, double rtol, double abstol, double dtol, int32_t max_it);
// One CG iteration (+ the V-cycle) on st; every kernel is a no-op once the
// device stop flag is set, every collective is issued regardless.
int cg_iteration(const CGRun &R, hipStream_t st);
// KSPSolve_CG on the caller's stream; the results land in cg.
int cg_solve(CGSolve &cg, CGOperator &op, const double *b, double *x, hipStream_t s);
