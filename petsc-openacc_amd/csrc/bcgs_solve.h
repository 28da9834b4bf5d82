// bcgs_solve.h — the preconditioned BiCGStab driver (bcgs_solve.hip) of the
// single-GPU handle (ksp.hip). It runs on the CG driver's CGSolve (tolerances,
// D^-1, R / P / W, the partial lists, the history and the last solve's
// results) and CGOperator (product, V-cycle, wait), plus the vectors BiCGStab
// has beyond CG's. Not part of the ABI.
#pragma once

#include "bcgs_device.h"
#include "cg_solve.h"

// BiCGStab's own device vectors (RP, V, S, T) and scalar state.
struct BCGSWork {
    int64_t m = -1;  // rows the vectors are allocated for (-1: none)
    double *d_rp = nullptr, *d_v = nullptr, *d_s = nullptr, *d_t = nullptr;
    BCGSState *d_state = nullptr;
    BCGSState *h_state = nullptr;  // pinned
};

// Allocate the work vectors for m rows (a no-op when they are there).
int bcgs_reserve(BCGSWork &bw, int64_t m);
void bcgs_free(BCGSWork &bw);
// One BiCGStab iteration on st; every kernel is a no-op once the device stop
// flag is set.
int bcgs_iteration(CGSolve &cg, BCGSWork &bw, CGOperator &op, double *x, const CGParams &p, hipStream_t st);
// KSPSolve_BCGS on the caller's stream, on a set-up cg and reserved bw; the
// results land in cg (its, reason, rnorm, hist, waits).
int bcgs_solve(CGSolve &cg, BCGSWork &bw, CGOperator &op, const double *b, double *x, hipStream_t s);
