// cg_multi.h — KSPMatSolve on the single-GPU handle: k independent
// preconditioned CG recurrences advanced in lock step on MatMatMult
// (cg_multi.hip). Column j is cg_solve.hip's unfused single-vector solve bit
// for bit; the columns share one pass over the matrix per chunk of columns
// and nothing else. Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "cg_solve.h"
#include "mg_cycle.h"

// The lock-step work vectors (m x k interleaved, leading dimension = the
// solve's k), the per-column partial lists, states and histories, and the
// last mat_solve's results. Owned by the handle: allocated on the first call
// for a width, regrown when k (or the history) grows, freed with the set-up.
struct CGMulti {
    int32_t cap_k = 0;     // columns the allocations hold
    int32_t hist_cap = 0;  // entries of one column's history
    int64_t m = 0;
    int nb = 0;            // vector-kernel blocks = partials per quantity and column
    double *d_r = nullptr, *d_z = nullptr, *d_p = nullptr, *d_part = nullptr, *d_hist = nullptr;
    CGState *d_state = nullptr;
    int *d_flag = nullptr;       // 1 once every column is done
    CGState *h_state = nullptr;  // pinned, cap_k states
    int *h_flag = nullptr;       // pinned
    // the last mat_solve
    int32_t k = 0;
    std::vector<int32_t> its;
    std::vector<int> reason;
    std::vector<double> rnorm;
    std::vector<std::vector<double>> hist;
};

// The handle's GAMG hierarchy and its multi-column level blocks (mg_cycle.h)
struct CGMultiPC {
    const std::vector<aijhip::MGLevelView> *lv;
    const aijhip::MGMultiBlocks *mb;
};

void cgm_free(CGMulti &mm);
// The work vectors for k columns (cgm_solve calls it; a handle with a reserved
// V-cycle width calls it at set-up, so that its solves allocate nothing).
int cgm_reserve(const CGSolve &cg, CGMulti &mm, int32_t k);
// dst = src for an m x k block between layouts / leading dimensions (sil, dil:
// interleaved), one lane per entry, on s.
void cgm_copy_block(int64_t m, int32_t k, int n_cu, const double *src, int64_t lds, bool sil, double *dst,
                    int64_t ldd, bool dil, hipStream_t s);
// A X = B for k columns on s with cg's tolerances, norm type, initial-guess
// flag, poll and PC (none / Jacobi, or with mg the GAMG V-cycle on blocks
// reserved for k columns; cg must be set up for A). B and X are checked by
// the caller. The per-column results land in mm, column k - 1's
// and the polls also in cg (its, reason, rnorm, hist, waits).
int cgm_solve(CGSolve &cg, CGMulti &mm, const aijhip_mat &A, int32_t k, int layout, const double *B, int64_t ldb,
              double *X, int64_t ldx, hipStream_t s, const CGMultiPC *mg = nullptr);
