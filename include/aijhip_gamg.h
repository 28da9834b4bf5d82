/*
 * aijhip_gamg.h — smoothed-aggregation multigrid hierarchy (the PCGAMG the
 * reference configures: /root/reference/configs/PETSc_SolverOptions_GAMG.info
 * :6-21, -pc_gamg_type agg -pc_gamg_agg_nsmooths 1 -pc_gamg_threshold 0.0;
 * SURVEY.md §8f row 3).
 *
 * The hierarchy is built on the host ("setup can stay on the
 * host") by the same steps as PETSc 3.7's PCSetUp_GAMG with the agg type
 * [ext]: strength graph |a_ij| > threshold*sqrt(|a_ii a_jj|), i != j;
 * aggregation; tentative prolongator from the near-null space (constant
 * vector on the finest level; the QR factors carry it down); one Jacobi
 * smoothing step P = (I - 1.4/emax D^-1 A) P0 (PCGAMGOptProlongator_AGG's
 * alpha = -1.4/emax); Galerkin coarse operator Pt A P. Aggregation:
 * PETSc 3.7's own agg coarsening restated (coarsen 1, the default since
 * round 5: a maximal independent set of the squared graph in a hashed random
 * order, aggregates smoothed — agg.c PCGAMGCoarsen_AGG / smoothAggs, mis.c;
 * PETSc's random stream is not reproduced) or a deterministic greedy pass in
 * natural order (coarsen 0, the default through round 4), with emax from
 * CG's Lanczos tridiagonal as PCGAMGOptProlongator_AGG does (eig_ksp 1, the
 * default) or a power iteration (eig_ksp 0). GAMG iteration parity with
 * PETSc is unpinned either way (PETSc is absent). The distributed set-up
 * (PCGAMG across ranks) takes the same parameters, its MIS on each rank's
 * diagonal block.
 * The solve-phase V-cycle runs on the device inside aijhip_ksp
 * (AIJHIP_PC_GAMG), whose set-up builds the large levels on the device
 * (device_min_rows) with results identical to aijhip_gamg_build_host.
 */
#ifndef AIJHIP_GAMG_H
#define AIJHIP_GAMG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct aijhip_gamg_params {
    double threshold;        /* -pc_gamg_threshold (0.0)                     */
    int32_t coarse_eq_limit; /* -pc_gamg_coarse_eq_limit (50)                */
    int32_t max_levels;      /* -pc_mg_levels (10)                           */
    int32_t nsmooths;        /* -pc_gamg_agg_nsmooths (1)                    */
    double smooth_scale;     /* 1.4 in alpha = -smooth_scale / emax          */
    int32_t eig_its;         /* iterations of the emax(D^-1 A) estimate (10) */
    int32_t threads;         /* host threads for set-up (0 = OpenMP default) */
    int32_t device_min_rows; /* KSP set-up: levels with at least this many rows
                              * (or 25 x as many entries) are built on the
                              * device (strength graph, emax, aggregation,
                              * smoothing, Galerkin product); smaller ones on
                              * the host.
                              * 0 = every level on the device, INT32_MAX = all
                              * on the host. Same hierarchy either way.     */
    /* ABI 3: */
    int32_t coarsen;         /* 1 (default): PETSc 3.7 agg's MIS (see above);
                              * 0: greedy aggregation (natural order)       */
    int32_t square_graph;    /* -pc_gamg_square_graph (1): coarsen 1 squares
                              * the graph on this many levels from the finest */
    int32_t eig_ksp;         /* emax(D^-1 A): 1 (default) CG's Lanczos estimate,
                              * PETSc's; 0 power iteration                   */
    int32_t pad0;
} aijhip_gamg_params_t;

typedef struct aijhip_gamg_host *aijhip_gamg_host_t;

int aijhip_gamg_params_default(aijhip_gamg_params_t *p);

/* The level smoother of the V-cycle (every level but the coarsest, which stays
 * preonly + Jacobi; the same down and up), after PETSc 3.7's
 * KSPSolve_Richardson / KSPSolve_Chebyshev with a Jacobi PC [ext]:
 *   Richardson(its), scale s: x = s D^-1 b from a zero guess, then
 *     x = x + s D^-1 (b - A x). its = 1, s = 1 is the default.
 *   Chebyshev(its) on D^-1 A over [emin, emax] = [lo, hi] x the level's
 *     emax(D^-1 A) estimate (the one the set-up makes to smooth the
 *     prolongator: it needs nsmooths > 0), PETSc's GAMG default. With
 *     scale and omega_i from aijhip_mg_cheby_coefficients:
 *       p_0 = scale D^-1 b (zero guess) or x + scale D^-1 (b - A x),
 *       p_(i+1) = ((1 - omega_i) p_(i-1) + omega_i p_i)
 *                 + omega_i scale D^-1 (b - A p_i),  p_(-1) = the guess,
 *     the result p_its: its products down, its + 1 up. */
enum { AIJHIP_MG_SMOOTH_RICHARDSON = 0, AIJHIP_MG_SMOOTH_CHEBYSHEV = 1 };
#define AIJHIP_MG_MAX_ITS 16
typedef struct aijhip_mg_smoother {
    int32_t type;             /* -mg_levels_ksp_type (RICHARDSON)             */
    int32_t its;              /* -mg_levels_ksp_max_it (1), 1..16             */
    double richardson_scale;  /* -mg_levels_ksp_richardson_scale (1.0)        */
    double cheby_lo, cheby_hi;/* emin = lo*emax_est, emax = hi*emax_est (0.05, 1.05) */
} aijhip_mg_smoother_t;
int aijhip_mg_smoother_default(aijhip_mg_smoother_t *s);
/* The Chebyshev schedule for its = k steps on [emin, emax], in double:
 *   scale = 2/(emax+emin); alpha = 1 - scale*emin; mu = 1/alpha;
 *   c_(-1) = 1, c_0 = mu, c_(i+1) = 2 mu c_i - c_(i-1),
 *   omega_i = (2/alpha) c_i / c_(i+1)   (omega[0..k)). */
int aijhip_mg_cheby_coefficients(double emax, double emin, int32_t k, double *scale, double *omega);

/* Build the hierarchy for the square CSR operator (host arrays). Level 0 is
 * the input operator; level l+1 = Pt_l A_l P_l. */
int aijhip_gamg_build_host(int32_t m, const int32_t *ai, const int32_t *aj, const double *aa,
                           const aijhip_gamg_params_t *p, aijhip_gamg_host_t *out);
int aijhip_gamg_host_num_levels(aijhip_gamg_host_t h, int32_t *nlevels);
/* Sizes of level l: rows, nnz of A_l; for l < nlevels-1 also nnz of P_l
 * (rows m_l, columns m_{l+1}) and the emax estimate used to smooth it. */
int aijhip_gamg_host_level_info(aijhip_gamg_host_t h, int32_t l, int32_t *m, int64_t *nnz_a,
                                int64_t *nnz_p, double *emax);
/* Copy out level l's operator (l >= 1), interpolation P_l, aggregates of
 * level l's rows (agg[i] = coarse row), into caller arrays sized by
 * level_info. */
int aijhip_gamg_host_get_A(aijhip_gamg_host_t h, int32_t l, int32_t *ai, int32_t *aj, double *aa);
int aijhip_gamg_host_get_P(aijhip_gamg_host_t h, int32_t l, int32_t *ai, int32_t *aj, double *aa);
int aijhip_gamg_host_get_aggregates(aijhip_gamg_host_t h, int32_t l, int32_t *agg);
/* Borrow level l's operator (which = 'A', l >= 1) or interpolation
 * (which = 'P', l < nlevels-1) in place: the pointers stay valid until
 * aijhip_gamg_host_destroy (no copy; the device set-up uploads from them). */
int aijhip_gamg_host_view(aijhip_gamg_host_t h, int32_t l, char which, const int32_t **ai, const int32_t **aj,
                          const double **aa);
int aijhip_gamg_host_destroy(aijhip_gamg_host_t h);

/* ---- Diagnostics ----
 * The device set-up's sparse products and prolongator parts on host operands:
 * each call uploads its arguments, runs the set-up's own device routine
 * unchanged on the current device and keeps the result on the host, in a
 * handle read with the getters below (CSR results) or in the caller's arrays.
 * Operands are CSR with int32 offsets; a B row holds every column at most
 * once (the products' precondition, not checked), an A row may repeat one. */
typedef struct aijhip_gamg_diag *aijhip_gamg_diag_t;

/* C = A B, A m x k, B k x n, by the hash-table product the Galerkin operators
 * are built with. n_cu: the compute-unit count the product sizes its grid and
 * its tables by (0 = the device's own). AIJHIP_ERR_STATE when a row of C has
 * more distinct columns than the largest table holds (the set-up then builds
 * the level on the host); *out is NULL then. */
int aijhip_gamg_diag_rowprod(int32_t m, int32_t k, int32_t n, const int32_t *ai, const int32_t *aj,
                             const double *aa, const int32_t *bi, const int32_t *bj, const double *ba,
                             int32_t n_cu, aijhip_gamg_diag_t *out);
/* T = A P0, A m x k, P0 k x na with one entry per row: column agg[j], value
 * p0[j], none where agg[j] = -1 (the product the prolongator is smoothed
 * with: its register form, or the hash-table product when a row has more
 * than 8 distinct columns or A more than 8 entries per row). */
int aijhip_gamg_diag_rowprod_p0(int32_t m, int32_t k, int32_t na, const int32_t *ai, const int32_t *aj,
                                const double *aa, const int32_t *agg, const double *p0, int32_t n_cu,
                                aijhip_gamg_diag_t *out);
/* P = P0 + alpha D^-1 T on the union pattern: T m x n with ascending columns,
 * P0's row i the entry (agg[i], p0[i]) or none (agg[i] = -1), dinv[i] = 1/d_i. */
int aijhip_gamg_diag_prolong(int32_t m, int32_t n, const int32_t *ti, const int32_t *tj, const double *ta,
                             const int32_t *agg, const double *p0, const double *dinv, double alpha,
                             aijhip_gamg_diag_t *out);
/* The tentative prolongator of the near-null space B[0, m) over aggregates
 * agg[i] in [-1, na): s2[a] = the sum of B_i^2 over a's members in ascending
 * i, Bc[a] = its square root, p0[i] = B[i] / Bc[agg[i]] (0 where Bc is 0 or
 * agg[i] = -1). b_ones != 0: B is all 1.0 (the finest level's form). */
int aijhip_gamg_diag_tentative(int32_t m, int32_t na, const int32_t *agg, const double *B, int32_t b_ones,
                               double *Bc, double *p0, double *s2);
/* C = A B where C's pattern is known: ci (m + 1 offsets) and cj, ascending in
 * every row and holding every column the product reaches (the pattern of
 * aijhip_gamg_diag_rowprod on operands of the same structure; it may hold
 * more). Only the values are computed, by the numeric-only kernel the GAMG
 * refresh uses: each C(i, j) from +0.0, the products a_ik b_kj rounded and
 * added in traversal order, a pattern column no product reaches left +0.0 —
 * the bits of aijhip_gamg_diag_rowprod on the same operands. The rows go by
 * their pattern length to a class of that capacity (aijhip_gamg_diag_get_passes:
 * lanes, capacity, 1, capacity per launch); AIJHIP_ERR_STATE when a row holds
 * 1024 columns or more (the refresh sends such a level to the host). */
int aijhip_gamg_diag_rowprod_numeric(int32_t m, int32_t k, int32_t n, const int32_t *ai, const int32_t *aj,
                                     const double *aa, const int32_t *bi, const int32_t *bj, const double *ba,
                                     const int32_t *ci, const int32_t *cj, int32_t n_cu, aijhip_gamg_diag_t *out);
/* Every (lanes per row, class capacity) pair the numeric-only kernel is
 * instantiated for: pairs[2 q], pairs[2 q + 1], up to cap pairs; *n = their
 * count. */
int aijhip_gamg_diag_numeric_classes(int32_t *pairs, int32_t cap, int32_t *n);
/* The result's rows, columns and entries; the hash-table launches recorded
 * (npasses); whether the register form of A P0 wrote the result. */
int aijhip_gamg_diag_info(aijhip_gamg_diag_t h, int32_t *m, int32_t *n, int64_t *nz, int32_t *npasses,
                          int32_t *p0_register);
int aijhip_gamg_diag_get_csr(aijhip_gamg_diag_t h, int32_t *ai, int32_t *aj, double *aa);
/* passes[4 p .. 4 p + 3] = lanes per row, table slots, mode (0 count, 1
 * write) and the most keys a row may hold in the table (keys_max) of launch
 * p, in launch order; row_table[i] = the slots of the table that wrote row i
 * (0: not a hash-table product). Either may be NULL. */
int aijhip_gamg_diag_get_passes(aijhip_gamg_diag_t h, int32_t *passes, int32_t *row_table);
int aijhip_gamg_diag_destroy(aijhip_gamg_diag_t h);

#ifdef __cplusplus
}
#endif

#endif /* AIJHIP_GAMG_H */
