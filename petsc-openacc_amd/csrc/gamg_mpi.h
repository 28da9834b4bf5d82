// gamg_mpi.h — PCGAMG across ranks (gamg_mpi.hip), used by the distributed
// KSP (ksp_mpi.hip) for AIJHIP_PC_GAMG at more than one rank.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "aijhip.h"
#include "aijhip_gamg.h"
#include "aijhip_mpi.h"
#include "mg_cycle.h"

namespace aijhip_gamg_mpi {

// One level of the distributed hierarchy on this rank: what the V-cycle
// reads of it (the view it extends: m own rows, A = [Ad | Ao] with Ao's
// columns the slots of op's ghost vector, op = MatMult_MPIAIJ + the level's
// p2p halo (level 0: the caller's), D^-1 and the level vectors) and the
// set-up's ownership data. Transfer to level l+1: P = [Pd | Po] (Po's
// columns: level l+1's ghost slots); R = P^T as MatMultTranspose_MPIAIJ:
// Pd^T (attached to Pd) and Po^T (attached to Po) whose ghost-slot sums go
// back to their owners.
struct Level : aijhip::MGLevelView {
    int64_t rstart = 0;            // first global row
    std::vector<int64_t> starts;   // ownership: rank q owns [starts[q], starts[q+1])
    std::vector<int64_t> ghost_gid;  // global row of every ghost slot
    double emax = 0.0;
};

struct Hierarchy {
    std::vector<Level> lv;  // finest first
    // what the V-cycle walks (aijhip::mg_vcycle): one multiplicative V-cycle
    // x = B b, every halo exchange issued on every rank whatever the stop
    // flag says, the kernels returning at once past it
    std::vector<aijhip::MGLevelView> view;
    void destroy();
};

// PCSetUp_GAMG over the distributed operator M0 (p2p halo). Collective.
// sm: the level smoother (its scalars and third vector go into each level's view).
int build(aijhip_mpiaij *M0, const aijhip_gamg_params_t &p, const aijhip_mg_smoother_t &sm, Hierarchy &H);
// This rank's rows of level l's operator ('A') or interpolation ('P') on the
// host, columns in the global numbering of their level (tests).
int get_level(const Hierarchy &H, int32_t l, char which, int64_t *rstart, int32_t *m, std::vector<int64_t> &ai,
              std::vector<int64_t> &aj, std::vector<double> &aa);

}  // namespace aijhip_gamg_mpi
