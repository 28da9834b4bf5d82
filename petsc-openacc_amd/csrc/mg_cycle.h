// mg_cycle.h — the one multigrid V-cycle (mg_cycle.hip) over a per-level
// view that each hierarchy fills at set-up: the single-GPU PCGAMG (ksp.hip)
// and the distributed one (gamg_mpi.hip). Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "aijhip_gamg.h"
#include "aijhip_internal.h"

struct aijhip_mpiaij;

namespace aijhip {

struct MGLevelView {
    int32_t m = 0;  // own rows
    aijhip_mat *Ad = nullptr;  // the operator (own columns)
    aijhip_mat *Ao = nullptr;  // ghost columns (slots of op's ghost vector); NULL on one GPU
    // interpolation from level l+1 (NULL on the coarsest): P = [Pd | Po], the
    // restriction P^T as Pd->transpose and Po->transpose
    aijhip_mat *Pd = nullptr, *Po = nullptr;
    // MatMult_MPIAIJ + the halo of this level and of level l+1; NULL on one GPU
    aijhip_mpiaij *op = nullptr, *op_next = nullptr;
    double *dinv = nullptr;
    double *tdinv = nullptr;  // row templates: D^-1 per template (else NULL)
    double *b = nullptr, *x = nullptr, *r = nullptr;  // level 0: b and x are the caller's
    bool fused = false;  // smoothing passes fused into STREAM launches (AIJHIP_MG_UNFUSED=1: PETSc's order)
    // The level smoother (mg_set_smoother; the coarsest level ignores it):
    // Richardson(its) with rscale, or Chebyshev(its) on D^-1 A over
    // [cmin, cmax] with the host's scale and omega[0..its)
    int32_t smooth = AIJHIP_MG_SMOOTH_RICHARDSON, its = 1;
    double rscale = 1.0;
    double cmin = 0.0, cmax = 0.0, scale = 0.0, omega[AIJHIP_MG_MAX_ITS] = {};
    double *w = nullptr;  // one more level vector where the smoother rotates three (mg_smoother_needs_w)
};

// A smoother request checked (its in 1..AIJHIP_MG_MAX_ITS, 0 < lo < hi, a known
// type) and, at set-up (p != NULL), against the hierarchy's parameters:
// Chebyshev needs each level's emax(D^-1 A) estimate, which the set-up makes
// only to smooth the prolongator (nsmooths > 0). AIJHIP_ERR_ARG with a message.
int mg_check_smoother(const aijhip_mg_smoother_t &s, const aijhip_gamg_params_t *p = nullptr);
// Fills L's smoother fields from the request and the level's emax(D^-1 A)
// estimate lambda (Chebyshev: bounds lo * lambda, hi * lambda and the
// coefficient schedule of aijhip_mg_cheby_coefficients).
int mg_set_smoother(const aijhip_mg_smoother_t &s, double lambda, MGLevelView &L);
// Whether a smoothed level with L's smoother and `fused` needs L.w.
bool mg_smoother_needs_w(const MGLevelView &L);

// PCApply_MG (multiplicative, one V-cycle): x0 = B b0 on `s`. Every kernel
// takes CG's stop flag (NULL outside a solve) and returns at once past it;
// every halo exchange is issued on every rank regardless. With dots != NULL a
// fused finest post-smoothing that can carry them leaves the z.z / z.b
// partials there (2 x its STREAM blocks; *dots_done = true).
int mg_vcycle(const std::vector<MGLevelView> &lv, const double *b0, double *x0, hipStream_t s, const int *stop,
              double *dots = nullptr, bool *dots_done = nullptr);

// The multi-column V-cycle's level blocks: b, x, r and w of every level, m_l x
// cap_k interleaved (a cycle of k <= cap_k columns uses leading dimension k).
// Level 0's b and x are staging for callers whose blocks are not tight
// interleaved. Owned by the handle (aijhip_ksp_set_mat_vcycle_width).
struct MGMultiBlocks {
    struct Level {
        double *b = nullptr, *x = nullptr, *r = nullptr, *w = nullptr;
    };
    int32_t cap_k = 0;
    std::vector<Level> lev;
};
int mg_multi_reserve(const std::vector<MGLevelView> &lv, int32_t kmax, MGMultiBlocks &mb);
void mg_multi_free(MGMultiBlocks &mb);

// PCMatApply_MG on one GPU (op, Ao, Po NULL on every level): one V-cycle on
// the k columns of the tight interleaved m x k blocks B0 -> X0 (leading
// dimension k), column j entry for entry mg_vcycle on column j: the same
// smoothers, zero-guess starts and coarse solve, every smoothing step and
// residual one launch_spmm with its epilogue on every level (no unfused form;
// AIJHIP_MG_UNFUSED does not reach it), restriction launch_spmm(plain) on
// Pd->transpose, interpolation launch_spmm(add) on Pd. Going down the steps
// rotate x and w, coming up x and r, from a first buffer chosen by the parity
// of the step count, so the result lands in X0 without a copy and a step's
// result never aliases the operand it gathers.
int mg_vcycle_multi(const std::vector<MGLevelView> &lv, const MGMultiBlocks &mb, int32_t k, const double *B0,
                    double *X0, hipStream_t s, const int *stop);

}  // namespace aijhip
