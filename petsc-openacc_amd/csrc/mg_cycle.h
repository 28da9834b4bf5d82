// mg_cycle.h — the one multigrid V-cycle (mg_cycle.hip) over a per-level
// view that each hierarchy fills at set-up: the single-GPU PCGAMG (ksp.hip)
// and the distributed one (gamg_mpi.hip). Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

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
};

// PCApply_MG (multiplicative, one V-cycle): x0 = B b0 on `s`. Every kernel
// takes CG's stop flag (NULL outside a solve) and returns at once past it;
// every halo exchange is issued on every rank regardless. With dots != NULL a
// fused finest post-smoothing that can carry them leaves the z.z / z.b
// partials there (2 x its STREAM blocks; *dots_done = true).
int mg_vcycle(const std::vector<MGLevelView> &lv, const double *b0, double *x0, hipStream_t s, const int *stop,
              double *dots = nullptr, bool *dots_done = nullptr);

}  // namespace aijhip
