/*
 * aijhip_ksp.h — device-resident Krylov solve around the MI355X SpMV
 * (the caller of MatMult_SeqAIJ in the reference,
 * /root/reference/src/main_ksp.cpp:92-103 with
 * /root/reference/configs/PETSc_SolverOptions_GAMG.info:1-4).
 *
 * Mirrors PETSc 3.7.6's KSPSolve_CG [ext] (src/ksp/ksp/impls/cg/cg.c) and
 * KSPConvergedDefault [ext] (src/ksp/ksp/interface/iterativ.c): preconditioned
 * CG with the preconditioned residual norm by default, the same breakdown
 * checks (beta = 0, indefinite PC, indefinite matrix) and the same reason
 * codes. Vectors are device arrays; all scalar work (alpha, beta, the
 * convergence test) runs on the device, so iterations are launched without a
 * host round trip. Dot products are reduced in a fixed order (deterministic
 * run to run) but not in BLAS ddot's order, so results match PETSc to
 * rounding, not bit for bit.
 */
#ifndef AIJHIP_KSP_H
#define AIJHIP_KSP_H

#include <stdint.h>

#include "aijhip.h"
#include "aijhip_gamg.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct aijhip_ksp *aijhip_ksp_t;

/* PCType: PCNONE, PCJACOBI (= bjacobi + jacobi sub-PC on one rank,
 * PETSc_SolverOptions_GAMG.info:16-21), PCGAMG (agg, one V-cycle per
 * application: Richardson(1) + Jacobi smoothing down and up on every level
 * unless aijhip_ksp_set_mg_smoother chose another smoother,
 * preonly + Jacobi on the coarsest — PETSc_SolverOptions_GAMG.info:6-21;
 * hierarchy from include/aijhip_gamg.h). */
enum {
    AIJHIP_PC_NONE = 0,
    AIJHIP_PC_JACOBI = 1,
    AIJHIP_PC_GAMG = 2,         /* PCGAMG; on a distributed operator (aijhip_kspmpi,
                                   more than one rank) the hierarchy spans the
                                   ranks, as PETSc's agg GAMG does             */
    AIJHIP_PC_BJACOBI_GAMG = 3  /* distributed operator only: -pc_type bjacobi
                                   -sub_pc_type gamg (one hierarchy per rank's
                                   diagonal block, no coupling)               */
};

/* KSPNormType values as in PETSc. */
enum {
    AIJHIP_KSP_NORM_NONE = 0,
    AIJHIP_KSP_NORM_PRECONDITIONED = 1,
    AIJHIP_KSP_NORM_UNPRECONDITIONED = 2,
    AIJHIP_KSP_NORM_NATURAL = 3
};

/* KSPConvergedReason values as in PETSc 3.7. */
enum {
    AIJHIP_KSP_CONVERGED_ITERATING = 0,
    AIJHIP_KSP_CONVERGED_RTOL = 2,
    AIJHIP_KSP_CONVERGED_ATOL = 3,
    AIJHIP_KSP_DIVERGED_ITS = -3,
    AIJHIP_KSP_DIVERGED_DTOL = -4,
    AIJHIP_KSP_DIVERGED_BREAKDOWN = -5, /* BiCGStab: v.rp = 0, t = 0 with s != 0, or rho = 0 */
    AIJHIP_KSP_DIVERGED_INDEFINITE_PC = -8,
    AIJHIP_KSP_DIVERGED_NANORINF = -9,
    AIJHIP_KSP_DIVERGED_INDEFINITE_MAT = -10
};

/* KSPCreate + KSPSetOperators(A, A) + KSPSetType(KSPCG) (aijhip_ksp_set_type
 * chooses another type). A must be square;
 * the handle borrows A (A must outlive it). Defaults as PETSc: rtol 1e-5,
 * atol 1e-50, dtol 1e5, max_it 10000, PC Jacobi, preconditioned norm,
 * zero initial guess. */
int aijhip_ksp_create(aijhip_mat_t A, aijhip_ksp_t *ksp);
int aijhip_ksp_set_tolerances(aijhip_ksp_t ksp, double rtol, double abstol, double dtol,
                              int32_t max_it);
int aijhip_ksp_set_pc_type(aijhip_ksp_t ksp, int pc_type);

/* KSPType: KSPCG (the default) and KSPBCGS. */
enum { AIJHIP_KSP_CG = 0, AIJHIP_KSP_BCGS = 1 };

/* KSPSetType / KSPGetType. An unknown type is AIJHIP_ERR_ARG. A change of type
 * keeps the PC: a GAMG hierarchy that is set up stays set up
 * (aijhip_ksp_get_gamg_setup_counts does not move); BiCGStab's extra work
 * vectors are allocated by the next aijhip_ksp_set_up or solve and freed with
 * the handle, so a solve on a handle that is set up allocates nothing.
 *
 * AIJHIP_KSP_BCGS: preconditioned BiCGStab for nonsymmetric operators, on the
 * device from the first residual to the last update. It restates PETSc 3.7.6
 * KSPSolve_BCGS [ext] (src/ksp/ksp/impls/bcgs/bcgs.c) with left
 * preconditioning, K(y) = B^-1 (A y) with B the handle's PC, and
 * KSPConvergedDefault [ext]:
 *
 *   x = 0 (or the caller's x);  r = B^-1 (b - A x);  dp = |r|;  hist[0] = dp
 *   converged(0, dp, snorm)     snorm = dp, or |B^-1 b| with a nonzero guess
 *   max_it <= 0: DIVERGED_ITS at iteration 0
 *   rp = r;  rhoold = alpha = omegaold = 1;  p = v = 0
 *   loop:  rho = r.rp;  beta = (rho / rhoold) (alpha / omegaold)
 *          p = r - (omegaold beta) v + beta p
 *          v = K(p);  d1 = v.rp;  d1 = 0: DIVERGED_BREAKDOWN (x untouched)
 *          alpha = rho / d1;  s = r - alpha v
 *          t = K(s);  d1 = s.t;  d2 = t.t
 *          d2 = 0: s.s != 0 is DIVERGED_BREAKDOWN; else x += alpha p,
 *                  its += 1, the norm is 0 and the reason CONVERGED_RTOL
 *          omega = d1 / d2;  x += alpha p + omega s;  r = s - omega t
 *          dp = |r|;  its += 1;  hist[its] = dp;  converged(its, dp)
 *          rho = 0: DIVERGED_BREAKDOWN;  its = max_it: DIVERGED_ITS
 *
 * One deliberate difference from PETSc: with max_it = 0 PETSc's do-while runs
 * one iteration; this solver stops at iteration 0 with DIVERGED_ITS, as this
 * library's CG does.
 *
 * Under AIJHIP_KSP_BCGS aijhip_ksp_solve, _solve_host and the getters of the
 * last solve (iteration number, residual norm, reason, history, host syncs)
 * serve BiCGStab; the tolerances, the initial-guess flag and AIJHIP_KSP_POLL
 * apply; aijhip_ksp_get_fused reports 0. Only the preconditioned norm is
 * served (the other norm types need right preconditioning): aijhip_ksp_solve
 * with another norm type returns AIJHIP_ERR_STATE before any device work, and
 * so do aijhip_ksp_mat_solve and _mat_solve_host, whose lock-step solver is
 * CG. aijhip_ksp_pc_apply and _pc_mat_apply do not depend on the type. */
int aijhip_ksp_set_type(aijhip_ksp_t ksp, int type);
int aijhip_ksp_get_type(aijhip_ksp_t ksp, int *type);
int aijhip_ksp_set_norm_type(aijhip_ksp_t ksp, int norm_type);
int aijhip_ksp_set_initial_guess_nonzero(aijhip_ksp_t ksp, int flg);
/* KSPSetUp: PC set-up (inverse diagonal) and work vectors. Called by solve
 * if needed; call it explicitly to time set-up apart from the solve. */
int aijhip_ksp_set_up(aijhip_ksp_t ksp);
/* KSPSolve: b, x device fp64[m]; x is overwritten (zeroed first unless the
 * initial guess is nonzero). Returns once the solve has finished. */
int aijhip_ksp_solve(aijhip_ksp_t ksp, const double *b, double *x, void *stream);
/* KSPSolve with HOST vectors b, x (fp64[m]; x is also read when the initial
 * guess is nonzero): b goes up and x comes down once per solve, the whole
 * solve runs on the device — the solve-level offload an unchanged PETSc
 * caller with host Vecs reaches through a registered KSP type
 * (petsc-openacc_amd/petsc/aijhip_ksp_petsc.c), instead of two PCIe copies per
 * MatMult. Synchronous. */
int aijhip_ksp_solve_host(aijhip_ksp_t ksp, const double *b, double *x);
int aijhip_ksp_get_iteration_number(aijhip_ksp_t ksp, int32_t *its);
int aijhip_ksp_get_residual_norm(aijhip_ksp_t ksp, double *rnorm);
int aijhip_ksp_get_converged_reason(aijhip_ksp_t ksp, int *reason);
/* KSPGetResidualHistory: copies min(na, its + 1) norms; *n = that count. */
int aijhip_ksp_get_residual_history(aijhip_ksp_t ksp, double *hist, int32_t na, int32_t *n);
/* Fused kernels used per iteration (1 = SpMV with the p.Ap dot in its
 * epilogue), for reporting. */
int aijhip_ksp_get_fused(aijhip_ksp_t ksp, int *fused);
/* Host synchronisations made by the last solve: the polls of the device stop
 * flag (one per batch of 8 iterations, AIJHIP_KSP_POLL overrides) plus the
 * final read. */
int aijhip_ksp_get_host_syncs(aijhip_ksp_t ksp, int32_t *n);
/* Compulsory HBM bytes one CG iteration of the set-up solver moves (the
 * roofline of the solve): every SpMV at its plan's layout bytes
 * (aijhip_info_t.mult_layout_bytes: matrix, x once, y once) plus the vector
 * passes' reads and writes — CG's p = z + b p (with the deferred x += a p),
 * the r update, and for GAMG per level the Jacobi pass, the residual and
 * post-smoothing SpMVs with their b / D^-1 reads, MatRestrict (P^T),
 * MatInterpolateAdd (P, reading the level's x) and the coarse Jacobi.
 * With another level smoother (aijhip_ksp_set_mg_smoother) each smoothed
 * level of m rows adds, with D = 8 (1 where D^-1 is read through a row
 * template's id) and fused passes:
 *   Richardson(k): 2 (k - 1) products of A_l, each with (8 + D) m of row
 *     operands (b, D^-1);
 *   Chebyshev(k): 2 k products of A_l: down, the first step (8 + D) m (b,
 *     D^-1) and each later one (16 + D) m (p_(i-1) too); up, the start
 *     (8 + D) m — the one post-smoothing product the default already counts —
 *     and each of the k steps (16 + D) m.
 * Unfused levels (AIJHIP_MG_UNFUSED=1): each added product is followed by a
 * vector pass of 40 m (Richardson, Chebyshev's start and first step down) or
 * 48 m (the other Chebyshev steps).
 * The per-part split: *spmv_bytes of the total are matrix launches, *level0
 * of the total belong to the finest level (its SpMVs and vectors). Valid
 * after set-up; the first iteration moves a little less.
 *
 * A BiCGStab handle (AIJHIP_KSP_BCGS) reports one BiCGStab iteration, with m
 * rows: two products at mult_layout_bytes each, two PC applications (GAMG:
 * two V-cycles, each counted as above) and the five vector passes
 *   p = r - (omegaold beta) v + beta p        32 m  (reads r, p, v; writes p)
 *   v = D^-1 v with the v.rp partials         32 m  (reads v, D^-1, rp; writes v;
 *                                                    none / GAMG 16 m: reads v, rp)
 *   s = r - alpha v                           24 m  (reads r, v; writes s)
 *   t = D^-1 t with s.t, t.t, s.s             32 m  (reads t, D^-1, s; writes t;
 *                                                    none / GAMG 16 m: reads t, s)
 *   x += alpha p + omega s, r = s - omega t   56 m  (reads x, p, s, t, rp;
 *   with r.r, r.rp                                   writes x, r)
 *   *bytes = 2 mult_layout_bytes + 176 m (Jacobi), + 144 m (none, and GAMG
 *   beside its two V-cycles). */
int aijhip_ksp_get_iteration_bytes(aijhip_ksp_t ksp, int64_t *bytes, int64_t *spmv_bytes, int64_t *level0);
/* GAMG options (before set-up); NULL = PETSc defaults
 * (aijhip_gamg_params_default). */
int aijhip_ksp_set_gamg_params(aijhip_ksp_t ksp, const aijhip_gamg_params_t *p);
/* The GAMG level smoother (aijhip_gamg.h; before set-up, a change clears it);
 * NULL = the default, Richardson(1) with scale 1. AIJHIP_ERR_ARG with a message
 * for its outside 1..16, lo <= 0, lo >= hi or an unknown type; Chebyshev with
 * nsmooths = 0 (no emax estimate) fails at set-up with AIJHIP_ERR_ARG. */
int aijhip_ksp_set_mg_smoother(aijhip_ksp_t ksp, const aijhip_mg_smoother_t *s);
/* The smoother of the set-up PC's level `level`: type, its and, for Chebyshev,
 * the bounds the level uses (lo, hi x its emax estimate; 0, 0 for Richardson).
 * Any out pointer may be NULL. */
int aijhip_ksp_get_mg_smoother(aijhip_ksp_t ksp, int32_t level, int32_t *type, int32_t *its, double *emin,
                               double *emax);
/* Multigrid levels of the set-up PC (1 for non-GAMG): rows and operator nnz
 * per level (finest first; up to cap entries), and the host set-up time. */
int aijhip_ksp_get_pc_levels(aijhip_ksp_t ksp, int32_t *nlevels, int32_t *rows, int64_t *nnz,
                             int32_t cap, double *setup_seconds);

/* Copy out GAMG level l's operator (which = 'A') or interpolation to level
 * l+1 ('P') from the device (PCMGGetSmoother / PCGetInterpolations
 * introspection): sizes into m, n, nnz; with ai == NULL only the sizes. */
int aijhip_ksp_get_pc_level(aijhip_ksp_t ksp, int32_t l, char which, int32_t *m, int32_t *n,
                            int64_t *nnz, int32_t *ai, int32_t *aj, double *aa);
/* How the GAMG set-up built each coarsening l -> l+1 (up to cap entries,
 * one per level but the coarsest): path[l] = 1 on the device
 * (aijhip_gamg build_device), 0 on the host builder; product_cols[l] = the
 * widest accumulator the device Galerkin products needed (0 = the wavefront
 * form, else 32 / 64 / 128 / 256 LDS columns per row; -1 on the host).
 * *host_fallback = 1 when a level the device would have built went to the
 * host because a product row exceeded 256 distinct columns. */
int aijhip_ksp_get_gamg_setup_path(aijhip_ksp_t ksp, int32_t cap, int32_t *path, int32_t *product_cols,
                                   int32_t *host_fallback);

/* -pc_gamg_reuse_interpolation [ext] (default 0: every change of the operator
 * takes the full set-up). With flg != 0, aijhip_ksp_set_up on a handle that is
 * set up with AIJHIP_PC_GAMG, whose operator has the sparsity structure it was
 * set up on (no aijhip_mat_assembly_end since) and new values or a new plan
 * (aijhip_mat_update_values / _device, aijhip_mat_set_option), REFRESHES the
 * hierarchy instead of rebuilding it. Kept: every P_l and P_l^T with their
 * handles and plans, the sparsity pattern of every A_l, the level vectors, the
 * multi-column blocks and the lock-step work vectors. Redone from the new
 * values: A_(l+1) = P_l^T (A_l P_l) into the existing level operators (the
 * numeric-only product: the sums in the set-up's order, the same bits as a
 * full product of the same operands), the level handles' value copies and
 * codes, D^-1 of every level, the fused-launch choices and the smoothers'
 * scalars; for Chebyshev each level's emax(D^-1 A_l) is estimated again with
 * the set-up's estimator, eig_its and eig_ksp. The prolongators keep the
 * smoothing they were built with. The pattern of each A_l P_l is kept on the
 * device between refreshes (made by the first refresh when the flag was set
 * on a handle already set up). A level with a row of 1024 columns or more in
 * A_l P_l or A_(l+1) is refreshed by the host builder's products on operands
 * read back from the device. (AIJHIP_GAMG_REFRESH=host is a test and
 * diagnostic switch: it sends every level of a handle there, for good on that
 * handle, so that the host path runs on small operands; the same bits.) A new
 * structure, PC type, GAMG parameters or
 * smoother still take the full set-up; PC none and Jacobi ignore the flag. A
 * refresh that fails leaves the handle not set up and returns the error; the
 * next set-up is a full one. */
int aijhip_ksp_set_gamg_reuse_interpolation(aijhip_ksp_t ksp, int flg);
int aijhip_ksp_get_gamg_reuse_interpolation(aijhip_ksp_t ksp, int *flg);
/* Set-ups this handle has run: full ones, refreshes, and the wall time of the
 * last of either kind. Any out pointer may be NULL. */
int aijhip_ksp_get_gamg_setup_counts(aijhip_ksp_t ksp, int32_t *full, int32_t *refreshed, double *last_seconds);
/* Diagnostics: the device addresses of what aijhip_ksp_set_mat_vcycle_width
 * reserves, for asserting that a call kept the allocations: per GAMG level
 * the multi-column blocks b, x, r, w (4 per level, finest first), then
 * KSPMatSolve's lock-step work vectors R, Z, P (0 where nothing is
 * allocated). Up to cap entries are written; *n = their count (4 levels + 3). */
int aijhip_ksp_get_mat_vcycle_reserve(aijhip_ksp_t ksp, int32_t cap, uint64_t *ptrs, int32_t *n);

#define AIJHIP_KSP_MAX_RHS 64

/* KSPMatSolve [ext]: A X = B, B and X m x k device blocks in one layout
 * (AIJHIP_DENSE_COLUMNS / AIJHIP_DENSE_INTERLEAVED, leading dimensions as in
 * aijhip_mat_mat_mult); elements outside the m x k blocks are neither read
 * nor written; B and X must not overlap.
 *
 * k independent CG recurrences advance in lock step, one iteration at a time,
 * the matrix read once per chunk of columns (aijhip_mat_mat_mult's chunks)
 * instead of once per column. Columns never mix (this is not block CG): each
 * has its own alpha, beta, norms, convergence test, reason, iteration count
 * and history, and a column that has stopped is frozen while the others go
 * on. The handle's tolerances, norm type, initial-guess flag and
 * AIJHIP_KSP_POLL apply to every column. Column j's X, iteration count,
 * reason and residual history equal, bit for bit, those of aijhip_ksp_solve
 * on that column with the dot products in passes of their own
 * (aijhip_ksp_get_fused = 0, e.g. an AIJHIP_KERNEL_SCALAR operator).
 *
 * PC none and Jacobi are served, and AIJHIP_PC_GAMG on a handle with a reserved
 * V-cycle width (aijhip_ksp_set_mat_vcycle_width, k within it): one
 * multi-column V-cycle per iteration, on all k columns until every column
 * has stopped (a stopped column's X, R, P and state stay frozen). Without a
 * reserved width a GAMG handle returns AIJHIP_ERR_STATE (the V-cycle has no
 * multi-column form), with k above it AIJHIP_ERR_STATE naming both. k = 0 does nothing;
 * k < 0 or k > AIJHIP_KSP_MAX_RHS, a NULL handle, a NULL B or X (m, k > 0), an
 * unknown layout, a leading dimension below the minimum and overlapping
 * blocks are AIJHIP_ERR_ARG, refused before any device work.
 *
 * Afterwards aijhip_ksp_get_iteration_number / _residual_norm /
 * _converged_reason / _residual_history report column k - 1 (what PETSc's
 * KSPMatSolve column loop leaves behind) and aijhip_ksp_get_host_syncs the
 * polls of this solve (one per batch of iterations plus the final read). */
int aijhip_ksp_mat_solve(aijhip_ksp_t ksp, int32_t k, int layout, const double *B, int64_t ldb,
                         double *X, int64_t ldx, void *stream);
/* The same with HOST blocks: upload, solve, download; synchronous. */
int aijhip_ksp_mat_solve_host(aijhip_ksp_t ksp, int32_t k, int layout, const double *B, int64_t ldb,
                              double *X, int64_t ldx);
/* Per column of the last mat_solve: up to cap entries each; *k = its width.
 * Any out pointer may be NULL. */
int aijhip_ksp_get_mat_solve_results(aijhip_ksp_t ksp, int32_t cap, int32_t *its, int *reason,
                                     double *rnorm, int32_t *k);
/* Column `column`'s residual history: copies min(na, its + 1) norms; *n = that
 * count. A column that stopped at the top of or inside iteration `its`
 * (DIVERGED_INDEFINITE_PC, DIVERGED_INDEFINITE_MAT, beta = 0) logged no norm
 * for it: its last entry is 0. */
int aijhip_ksp_get_mat_solve_history(aijhip_ksp_t ksp, int32_t column, double *hist, int32_t na, int32_t *n);
/* Compulsory HBM bytes of one lock-step iteration at width k on the set-up
 * handle (PC none / Jacobi), with m rows and c = the number of chunks k is cut
 * into (aijhip_mat_mat_mult_chunk_widths):
 *   P = Z + b P with the deferred X += a P   40 m k  (reads Z, P, X; writes P, X)
 *   W = A P                                  *spmm_bytes = aijhip_mat_mat_mult_get_plan's
 *                                            bytes at k interleaved columns (the matrix
 *                                            once per chunk, P in and W out once)
 *   the p . w partials                       16 m k  (reads P, W)
 *   R -= a W, Z = D^-1 R with their partials 32 m k  (reads R, W; writes R, Z)
 *                                            + 8 m c (Jacobi: D^-1 once per chunk)
 *   *bytes = *spmm_bytes + 88 m k (+ 8 m c).
 * At k = 1 this is at least aijhip_ksp_get_iteration_bytes - 16 m: the single
 * solver moves the same passes except that its fused dot saves the 16 m of
 * reading P and W again (and Jacobi on row templates stores no Z).
 *
 * A GAMG handle with a reserved width (k within it): *spmm_bytes = the CG
 * product and every product of the V-cycle at its
 * aijhip_mat_mat_mult_get_plan bytes (per smoothed level A_l 2 its times for
 * Richardson(its), 2 its + 2 for Chebyshev(its), P and P^T once), and
 *   CG's vector passes                        96 m k  (40 + 16 as above; R -= a W 24:
 *                                             reads R, W, writes R; the Z.Z, Z.R
 *                                             partials 16: reads Z, R)
 *   per level of m_l rows, x = f D^-1 b       16 m_l k + 8 m_l (the smoothers' start,
 *                                             the coarse solve)
 *   per smoothed level, the row operands the epilogues read beyond a product's
 *   own X and Y: residual 8 m_l k (b), interpolation 8 m_l k (x), a Richardson
 *   step 8 m_l k + 8 m_l c (b, D^-1 once per chunk), a Chebyshev step the same
 *   + 8 m_l k where it reads p_km1 (all but the first going down).
 * The matrices count once per chunk, so bytes(8) < 8 bytes(1). */
int aijhip_ksp_get_mat_solve_bytes(aijhip_ksp_t ksp, int32_t k, int64_t *bytes, int64_t *spmm_bytes);

/* The width the multi-column V-cycle is reserved for, 0 <= kmax <=
 * AIJHIP_KSP_MAX_RHS (default 0: KSPMatSolve and PCMatApply refuse a GAMG
 * handle). With kmax > 0 the hierarchy's level blocks (b, x, r, w of every
 * level, m_l x kmax) and KSPMatSolve's work vectors for kmax columns are
 * allocated at set-up; on a handle that is set up the call allocates them at
 * once and leaves the hierarchy as it is. A solve then allocates nothing
 * (the histories regrow only when max_it was raised). */
int aijhip_ksp_set_mat_vcycle_width(aijhip_ksp_t ksp, int32_t kmax);
int aijhip_ksp_get_mat_vcycle_width(aijhip_ksp_t ksp, int32_t *kmax);

/* PCApply [ext]: z = M^-1 r for the handle's PC (none: z = r; Jacobi:
 * z = D^-1 r; GAMG: one V-cycle), device vectors of m entries that do not
 * alias; sets the handle up if it is not. */
int aijhip_ksp_pc_apply(aijhip_ksp_t ksp, const double *r, double *z, void *stream);
/* PCMatApply [ext]: Z = M^-1 R for m x k device blocks in one layout, with
 * aijhip_ksp_mat_solve's argument checks and refusals (a GAMG handle needs a
 * reserved width of at least k). Column j of Z equals aijhip_ksp_pc_apply on
 * column j bit for bit wherever no level operator, P or P^T has a row of more
 * than 128 entries (longer rows are summed in another order by the
 * single-vector launches). For GAMG, blocks that are not tight interleaved
 * (columns layout, padded leading dimension) go through the handle's tight
 * interleaved blocks. Nothing outside the m x k block of Z is written. */
int aijhip_ksp_pc_mat_apply(aijhip_ksp_t ksp, int32_t k, int layout, const double *R, int64_t ldr, double *Z,
                            int64_t ldz, void *stream);

int aijhip_ksp_destroy(aijhip_ksp_t ksp);

#ifdef __cplusplus
}
#endif

#endif /* AIJHIP_KSP_H */
