// spmm.hip — MatMatMult_SeqAIJ_SeqDense [ext]: Y = A X for a block of k dense
// vectors, the matrix streamed once per chunk of W in {8, 4, 2, 1} columns
// instead of once per vector (aijhip_mat_mat_mult, include/aijhip.h).
//
// Every Y(i, j) is the PETSc row loop on column j: s = 0.0, then
// s += aa[p] * X(aj[p], j) in storage order, each product rounded before it is
// added (-ffp-contract=off) — the bits of oracle/matmult_seqaij.c on that
// column, for every path, layout, width and leading dimension. Unlike the
// default MatMult, a row of any length is summed by one lane in that order.
//
//  path 2, row templates (Plan::d_pid and d_pval): k_spmv_template's shape —
//          persistent workgroups over XCD chunks of the row blocks, the
//          templates' offsets and values staged in LDS once per workgroup;
//          neither aj nor aa is read.
//  path 1, CSR row blocks (STREAM plan, full rows, no long rows, block caps
//          <= 4096 entries): one workgroup per BlockDesc stages the block's aj
//          and aa in LDS with k_spmv_pattern's coalesced pair loads, then the
//          (row, column) tasks sum from LDS.
//  path 0, generic (everything else): one lane per (row, column) straight
//          from ai / aj / aa over all m rows; correctness only.
//
// Paths 1 and 2 deal a block's nrows x W (row, column) tasks to the lanes at
// lane stride T. Interleaved X: row = t / W, j = t % W — the W lanes of a row
// read the same LDS words and their gathers are W contiguous doubles. Column
// X: j = t / nrows, row = t % nrows — a wave's lanes walk down one column.
// All index arithmetic into X and Y is 64-bit.
//
// A launch may carry an epilogue (SpmmOp, aijhip_internal.h: MatMultAdd and the
// V-cycle's residual, Richardson and Chebyshev steps on interleaved blocks,
// the Ep* functors below) and a device stop flag past which every workgroup
// returns at once; without either it is EpPlain<false>, the launch as it was.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "aijhip_internal.h"

namespace aijhip {
namespace {

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef int i32x2 __attribute__((ext_vector_type(2)));

constexpr int kSpmmCap = 4096;      // entries of a path-1 block: 48 KiB of LDS (aj 16 + aa 32)
constexpr int kSpmmThreads = 512;   // path 1: three workgroups per CU in 160 KiB
constexpr int kSpmmTmplThreads = 256;
constexpr int kSpmmTmplTasks = 2;   // path 2: tasks a lane has in flight (k_spmv_template's R)
constexpr int kSpmmTmplWgPerCu = 8; // path 2: persistent workgroups per CU (32 waves, as template_grid)

// One chunk's W columns of X and Y (the pointers already at the chunk's first column)
template <bool IL>
struct Dense {
    const double *X;
    double *Y;
    int64_t ldx, ldy;
    __device__ const double *xp(int64_t i, int64_t j) const { return IL ? X + i * ldx + j : X + i + j * ldx; }
    __device__ double *yp(int64_t i, int64_t j) const { return IL ? Y + i * ldy + j : Y + i + j * ldy; }
};

// P columns of one row of X: one 8-byte load, or (P = 2, the pair variant: two
// adjacent interleaved columns from a 16-byte aligned address) one 16-byte load
template <int P>
__device__ __forceinline__ void ld_cols(const double *p, double (&v)[P]) {
    if constexpr (P == 2) {
        const f64x2 q = *reinterpret_cast<const f64x2 *>(p);
        v[0] = q.x;
        v[1] = q.y;
    } else {
        v[0] = *p;
    }
}
template <int P>
__device__ __forceinline__ void st_cols(double *p, const double (&v)[P]) {
    if constexpr (P == 2) {
        f64x2 q;
        q.x = v[0];
        q.y = v[1];
        __builtin_nontemporal_store(q, reinterpret_cast<f64x2 *>(p));
    } else {
        __builtin_nontemporal_store(v[0], p);
    }
}

// Task t of a block of nrows rows and G = W / P column groups
template <bool IL, int G>
__device__ __forceinline__ void task_of(int t, int nrows, int &row, int &jg) {
    if constexpr (IL) {
        row = t / G;
        jg = t % G;
    } else {
        jg = t / nrows;
        row = t % nrows;
    }
}

// What a launch does with a (row, column group)'s sums: the smoothing
// epilogues of the multi-column V-cycle (mg_vcycle_multi), the single-vector
// Ops of aijhip_kernels.hip (OpMult<true>, OpMgResid, OpMgPost, OpMgCheby) with
// the same expressions, parenthesised as there and nothing contracted. `row`
// loads the lane's row operands before the sum (B, PM1 and the result laid out
// as Y: `off` is the element's offset in Y; xo points at X(r, j), the gathered
// operand's own entry on a square operator), `seed` starts the sum, `put`
// stores and issues no load. Every workgroup returns at once past a set stop
// flag. STOP = false is the launch as it was: no flag is read.
template <bool STOP>
struct EpPlain {
    const int *stop;
    template <int P>
    struct Row {};
    __device__ bool stopped() const {
        if constexpr (STOP) return *stop != 0;
        else return false;
    }
    template <int P>
    __device__ void row(Row<P> &, const double *, int64_t, int64_t) const {}
    template <int P>
    __device__ void seed(double (&s)[P], const Row<P> &) const {
#pragma unroll
        for (int q = 0; q < P; ++q) s[q] = 0.0;
    }
    template <int P>
    __device__ void put(double *y, const double (&s)[P], const Row<P> &) const {
        st_cols<P>(y, s);
    }
};

// Y = Z + A X, MatMultAdd's order: the sum starts from Z(o, j) and the
// products are added to it in storage order (k_spmv_scalar's and the STREAM
// kernels' one-lane rows: sum = op.seed(o), then += in order). Z may be Y.
struct EpAdd {
    const int *stop;
    const double *Z;
    template <int P>
    struct Row {
        double z[P];
    };
    __device__ bool stopped() const { return stop && *stop != 0; }
    template <int P>
    __device__ void row(Row<P> &w, const double *, int64_t, int64_t off) const {
        ld_cols<P>(Z + off, w.z);
    }
    template <int P>
    __device__ void seed(double (&s)[P], const Row<P> &w) const {
#pragma unroll
        for (int q = 0; q < P; ++q) s[q] = w.z[q];
    }
    template <int P>
    __device__ void put(double *y, const double (&s)[P], const Row<P> &) const {
        st_cols<P>(y, s);
    }
};

// R = B + (-1) (A X) (OpMgResid)
struct EpResid {
    const int *stop;
    const double *B;
    template <int P>
    struct Row {
        double b[P];
    };
    __device__ bool stopped() const { return stop && *stop != 0; }
    template <int P>
    __device__ void row(Row<P> &w, const double *, int64_t, int64_t off) const {
        ld_cols<P>(B + off, w.b);
    }
    template <int P>
    __device__ void seed(double (&s)[P], const Row<P> &) const {
#pragma unroll
        for (int q = 0; q < P; ++q) s[q] = 0.0;
    }
    template <int P>
    __device__ void put(double *y, const double (&s)[P], const Row<P> &w) const {
        double v[P];
#pragma unroll
        for (int q = 0; q < P; ++q) v[q] = w.b[q] + (-1.0) * s[q];
        st_cols<P>(y, v);
    }
};

// X = T + sc (dinv_o (B + (-1) (A T))) (OpMgPost; sc = 1.0 multiplies to the
// bits of the literal form). The gathered operand is T; the result is not T.
struct EpPost {
    const int *stop;
    const double *B, *dinv;
    double sc;
    template <int P>
    struct Row {
        double t[P], b[P], di;
    };
    __device__ bool stopped() const { return stop && *stop != 0; }
    template <int P>
    __device__ void row(Row<P> &w, const double *xo, int64_t r, int64_t off) const {
        ld_cols<P>(xo, w.t);
        ld_cols<P>(B + off, w.b);
        w.di = dinv[r];
    }
    template <int P>
    __device__ void seed(double (&s)[P], const Row<P> &) const {
#pragma unroll
        for (int q = 0; q < P; ++q) s[q] = 0.0;
    }
    template <int P>
    __device__ void put(double *y, const double (&s)[P], const Row<P> &w) const {
        double v[P];
#pragma unroll
        for (int q = 0; q < P; ++q) v[q] = w.t[q] + sc * (w.di * (w.b[q] + (-1.0) * s[q]));
        st_cols<P>(y, v);
    }
};

// OUT = (c0 PM1 + c1 PK) + c2 (dinv_o (B + (-1) (A PK))), without PM1
// (NULL) c1 PK + that (OpMgCheby, both forms). The gathered operand is PK; OUT
// may be PM1's storage (a lane reads its own PM1 entries before it writes them),
// never PK's.
struct EpCheby {
    const int *stop;
    const double *B, *PM1, *dinv;
    double c0, c1, c2;
    template <int P>
    struct Row {
        double m[P], k[P], b[P], di;
    };
    __device__ bool stopped() const { return stop && *stop != 0; }
    template <int P>
    __device__ void row(Row<P> &w, const double *xo, int64_t r, int64_t off) const {
        if (PM1) ld_cols<P>(PM1 + off, w.m);
        ld_cols<P>(xo, w.k);
        ld_cols<P>(B + off, w.b);
        w.di = dinv[r];
    }
    template <int P>
    __device__ void seed(double (&s)[P], const Row<P> &) const {
#pragma unroll
        for (int q = 0; q < P; ++q) s[q] = 0.0;
    }
    template <int P>
    __device__ void put(double *y, const double (&s)[P], const Row<P> &w) const {
        double v[P];
#pragma unroll
        for (int q = 0; q < P; ++q) {
            const double corr = c2 * (w.di * (w.b[q] + (-1.0) * s[q]));
            v[q] = PM1 ? (c0 * w.m[q] + c1 * w.k[q]) + corr : c1 * w.k[q] + corr;
        }
        st_cols<P>(y, v);
    }
};

// Path 0: one lane per (row, column) over all m rows (compressed rows, long
// rows, SCALAR / VECTOR plans, the 16-wave geometries). An empty row gives +0.0.
template <bool IL, class E>
__global__ __launch_bounds__(256) void k_spmm_generic(int32_t m, int w, const int32_t *__restrict__ ai,
                                                      const int32_t *__restrict__ aj, const double *__restrict__ aa,
                                                      Dense<IL> D, E ep) {
    if (ep.stopped()) return;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)m * w) return;
    const int64_t row = IL ? t / w : t % m, j = IL ? t % w : t / m;
    const int64_t k1 = ai[row + 1];
    typename E::template Row<1> rw{};
    ep.template row<1>(rw, D.xp(row, j), row, D.yp(row, j) - D.Y);
    double s[1];
    ep.template seed<1>(s, rw);
    for (int64_t k = ai[row]; k < k1; ++k) s[0] += aa[k] * *D.xp(aj[k], j);
    ep.template put<1>(D.yp(row, j), s, rw);
}

// Path 1: one workgroup per row block. Phase 1 stages aj and aa of the block's
// entries [k0, k0 + nk), nk <= kSpmmCap, in LDS: 8-byte column pairs and 16-byte
// value pairs from an even start (the arrays' 2-entry tail pad keeps the last
// pair in bounds). Phase 2: the tasks sum from LDS in storage order, the loads
// of eight entries issued ahead of their dependent adds.
template <int W, bool IL, int P, class E>
__global__ __launch_bounds__(kSpmmThreads) void k_spmm_csr(const BlockDesc *__restrict__ blk,
                                                           const int32_t *__restrict__ ai,
                                                           const int32_t *__restrict__ aj,
                                                           const double *__restrict__ aa, Dense<IL> D, E ep) {
    static_assert(W % P == 0 && (P == 1 || IL), "the pair variant owns two adjacent interleaved columns");
    constexpr int T = kSpmmThreads, G = W / P;
    __shared__ double sa[kSpmmCap];
    __shared__ int32_t sj[kSpmmCap];
    if (ep.stopped()) return;
    const BlockDesc d = blk[blockIdx.x];
    if (d.nk < 0) return;
    const int t = threadIdx.x;
    const int64_t k0 = d.k0, k1 = (int64_t)d.k0 + d.nk;
    for (int64_t k = (k0 & ~int64_t(1)) + 2 * (int64_t)t; k < k1; k += 2 * T) {
        const i32x2 c = *reinterpret_cast<const i32x2 *>(aj + k);
        const f64x2 a = *reinterpret_cast<const f64x2 *>(aa + k);
        if (k >= k0) {
            sj[k - k0] = c.x;
            sa[k - k0] = a.x;
        }
        if (k + 1 < k1) {
            sj[k + 1 - k0] = c.y;
            sa[k + 1 - k0] = a.y;
        }
    }
    __syncthreads();
    const int ntask = d.nrows * G;
    for (int task = t; task < ntask; task += T) {
        int row, jg;
        task_of<IL, G>(task, d.nrows, row, jg);
        const int64_t r = (int64_t)d.row0 + row, j = (int64_t)jg * P;
        const int32_t rs = ai[r], n = ai[r + 1] - rs;
        const int32_t *cj = sj + (rs - d.k0);
        const double *ca = sa + (rs - d.k0);
        typename E::template Row<P> rw{};
        ep.template row<P>(rw, D.xp(r, j), r, D.yp(r, j) - D.Y);
        double s[P];
        ep.template seed<P>(s, rw);
        for (int32_t e0 = 0; e0 < n; e0 += 8) {
            double xv[8][P];
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (e0 + e < n) ld_cols<P>(D.xp(cj[e0 + e], j), xv[e]);
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (e0 + e < n) {
                    const double a = ca[e0 + e];
#pragma unroll
                    for (int q = 0; q < P; ++q) s[q] += a * xv[e][q];
                }
        }
        ep.template put<P>(D.yp(r, j), s, rw);
    }
}

// Path 2: k_spmv_template's persistent, XCD-chunked launch (workgroup g on XCD
// g % 8 takes the q-th eighth of the blocks, so the x planes a block gathers are
// in its own L2), the table of offsets and values staged in LDS once per
// workgroup. A lane has U tasks in flight; the ids of the block's next U tasks
// and the next blocks' descriptors are loaded while the current tasks gather.
// A task past the block's tasks has a row of length 0: it gathers nothing and
// does not store.
template <int W, bool IL, int P, class E>
__global__ __launch_bounds__(kSpmmTmplThreads) void k_spmm_template(const BlockDesc *__restrict__ blk, int nblk,
                                                                    const uint8_t *__restrict__ pid,
                                                                    const int32_t *__restrict__ ptab,
                                                                    const double *__restrict__ pval, int ntab,
                                                                    int npat, Dense<IL> D, E ep) {
    static_assert(W % P == 0 && (P == 1 || IL), "the pair variant owns two adjacent interleaved columns");
    constexpr int T = kSpmmTmplThreads, U = kSpmmTmplTasks, G = W / P;
    constexpr int TPT = (kPatTableMax + T - 1) / T;
    __shared__ int32_t tab[kPatTableMax];
    __shared__ double val[kPatTableMax];
    if (ep.stopped()) return;
    const int t = threadIdx.x, NG = (int)gridDim.x, g = (int)blockIdx.x;
    int first = g, step = NG, last = nblk;
    if (NG >= 8 && (NG & 7) == 0) {
        const int q = g & 7;
        first = (int)((int64_t)nblk * q / 8) + (g >> 3);
        step = NG >> 3;
        last = (int)((int64_t)nblk * (q + 1) / 8);
    }
    if (first >= last) return;
#pragma unroll
    for (int i = 0; i < TPT; ++i)
        if (t + i * T < ntab) {
            tab[t + i * T] = ptab[t + i * T];
            val[t + i * T] = pval[t + i * T];
        }
    BlockDesc d = blk[first], dn = d;
    if (first + step < last) dn = blk[first + step];
    __syncthreads();
    for (int b = first; b < last; b += step) {
        BlockDesc dnn = dn;
        if (b + 2 * step < last) dnn = blk[b + 2 * step];
        if (d.nk >= 0 && d.nrows > 0) {
            const int ntask = d.nrows * G;
            int row[U], jg[U], p[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                task_of<IL, G>(t + u * T, d.nrows, row[u], jg[u]);
                row[u] = min(row[u], d.nrows - 1);
                p[u] = pid[d.row0 + row[u]];
            }
            for (int base = 0; base < ntask; base += U * T) {
                int rown[U] = {}, jgn[U] = {}, pn[U] = {};
                if (base + U * T < ntask) {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        task_of<IL, G>(base + U * T + t + u * T, d.nrows, rown[u], jgn[u]);
                        rown[u] = min(rown[u], d.nrows - 1);
                        pn[u] = pid[d.row0 + rown[u]];
                    }
                }
                int st[U], n[U], nmax = 0;
                int64_t r[U], j[U];
                double s[U][P];
                typename E::template Row<P> rw[U] = {};
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool own = base + t + u * T < ntask;
                    const int32_t pm = tab[min(p[u], npat - 1)];
                    st[u] = pm & 0xffff;
                    n[u] = own ? pm >> 16 : 0;
                    nmax = max(nmax, n[u]);
                    r[u] = (int64_t)d.row0 + row[u];
                    j[u] = (int64_t)jg[u] * P;
                    if (own) ep.template row<P>(rw[u], D.xp(r[u], j[u]), r[u], D.yp(r[u], j[u]) - D.Y);
                    ep.template seed<P>(s[u], rw[u]);
                }
                for (int32_t e0 = 0; e0 < nmax; e0 += 8) {
                    double xv[U][8][P];
#pragma unroll
                    for (int u = 0; u < U; ++u)
#pragma unroll
                        for (int e = 0; e < 8; ++e)
                            if (e0 + e < n[u]) ld_cols<P>(D.xp(r[u] + tab[st[u] + e0 + e], j[u]), xv[u][e]);
#pragma unroll
                    for (int u = 0; u < U; ++u)
#pragma unroll
                        for (int e = 0; e < 8; ++e)
                            if (e0 + e < n[u]) {
                                const double a = val[st[u] + e0 + e];
#pragma unroll
                                for (int q = 0; q < P; ++q) s[u][q] += a * xv[u][e][q];
                            }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (base + t + u * T < ntask) ep.template put<P>(D.yp(r[u], j[u]), s[u], rw[u]);
                    row[u] = rown[u];
                    jg[u] = jgn[u];
                    p[u] = pn[u];
                }
            }
        }
        d = dn;
        dn = dnn;
    }
}

// The pair variant: each lane owns two adjacent interleaved columns and gathers
// them with one 16-byte load. It measured faster than the 8-byte form on both
// paths at every width it applies to (300^3, tools/spmm_ab.py, profiles/spmm/:
// CSR row blocks 564 / 787 / 1274 us against 648 / 943 / 1566 us at W = 2 / 4 /
// 8, row templates 469 / 943 / 1929 against 747 / 1531 / 3090 us), so it is what
// an interleaved chunk of two columns or more takes; AIJHIP_SPMM_PAIR=0 keeps
// the 8-byte form for A/B runs. A chunk takes it only when its X and Y are
// 16-byte aligned with even leading dimensions (no 16-byte access is ever
// issued at another address); otherwise, and for column blocks, the 8-byte form.
bool pair_wanted() {
    const char *v = std::getenv("AIJHIP_SPMM_PAIR");
    return !(v && *v) || std::atoi(v) != 0;
}

template <int W, bool IL, int P, class E>
hipError_t launch_chunk(const aijhip_mat &A, int path, const Dense<IL> &D, const E &ep, hipStream_t s) {
    const Plan &Pl = A.plan;
    if (path == kSpmmTemplate) {
        int g = (int)std::min<int64_t>(Pl.n_blocks, (int64_t)A.n_cu * kSpmmTmplWgPerCu);
        if (g >= 8) g &= ~7;
        hipLaunchKernelGGL((k_spmm_template<W, IL, P, E>), dim3(g), dim3(kSpmmTmplThreads), 0, s, Pl.d_blocks,
                           Pl.n_blocks, Pl.d_pid, Pl.d_ptab, Pl.d_pval, Pl.n_ptab, Pl.n_pat, D, ep);
    } else {
        hipLaunchKernelGGL((k_spmm_csr<W, IL, P, E>), dim3(Pl.n_blocks), dim3(kSpmmThreads), 0, s, Pl.d_blocks, A.d_ai,
                           A.d_aj, A.d_aa, D, ep);
    }
    return hipGetLastError();
}

// rowops: the epilogue's row operands (laid out as Y), which the pair variant
// reads with 16-byte loads too
template <int W, bool IL, class E>
hipError_t launch_width(const aijhip_mat &A, int path, const Dense<IL> &D, const E &ep, uintptr_t rowops,
                        hipStream_t s) {
    if (path == kSpmmGeneric) {
        const int64_t tasks = (int64_t)A.m * W;
        hipLaunchKernelGGL((k_spmm_generic<IL, E>), dim3((unsigned)((tasks + 255) / 256)), dim3(256), 0, s, A.m, W,
                           A.d_ai, A.d_aj, A.d_aa, D, ep);
        return hipGetLastError();
    }
    if (A.plan.n_blocks == 0) return hipSuccess;
    if constexpr (IL && W >= 2) {
        const bool aligned =
            ((reinterpret_cast<uintptr_t>(D.X) | reinterpret_cast<uintptr_t>(D.Y) | rowops) & 15) == 0 &&
            ((D.ldx | D.ldy) & 1) == 0;
        if (aligned && pair_wanted()) return launch_chunk<W, IL, 2, E>(A, path, D, ep, s);
    }
    return launch_chunk<W, IL, 1, E>(A, path, D, ep, s);
}

template <bool IL, class E>
hipError_t launch_layout(const aijhip_mat &A, int path, int w, const Dense<IL> &D, const E &ep, uintptr_t rowops,
                         hipStream_t s) {
    switch (w) {
        case 8: return launch_width<8, IL, E>(A, path, D, ep, rowops, s);
        case 4: return launch_width<4, IL, E>(A, path, D, ep, rowops, s);
        case 2: return launch_width<2, IL, E>(A, path, D, ep, rowops, s);
        default: return launch_width<1, IL, E>(A, path, D, ep, rowops, s);
    }
}

// One chunk's epilogue: the row operands at the chunk's first column (yo, Y's offset)
hipError_t launch_op(const aijhip_mat &A, int path, int w, const Dense<true> &D, const SpmmOp &op, int64_t yo,
                     const int *stop, hipStream_t s) {
    const double *B = op.B ? op.B + yo : nullptr, *M = op.PM1 ? op.PM1 + yo : nullptr;
    const uintptr_t rowops = reinterpret_cast<uintptr_t>(B) | reinterpret_cast<uintptr_t>(M);
    switch (op.op) {
        case kSpmmAdd: return launch_layout<true>(A, path, w, D, EpAdd{stop, B}, rowops, s);
        case kSpmmResid: return launch_layout<true>(A, path, w, D, EpResid{stop, B}, rowops, s);
        case kSpmmPost: return launch_layout<true>(A, path, w, D, EpPost{stop, B, op.dinv, op.c2}, rowops, s);
        case kSpmmCheby:
            return launch_layout<true>(A, path, w, D, EpCheby{stop, B, M, op.dinv, op.c0, op.c1, op.c2}, rowops, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

int spmm_path(const aijhip_mat &A) {
    const Plan &P = A.plan;
    if (P.kernel != AIJHIP_KERNEL_STREAM || A.compressed || P.n_longs != 0) return kSpmmGeneric;
    if (P.d_pid && P.d_pval) return kSpmmTemplate;
    if (P.tune.geom >= 0 && P.tune.geom < kNumStreamGeoms && kStreamGeoms[P.tune.geom].nnz_cap <= kSpmmCap)
        return kSpmmCsr;
    return kSpmmGeneric;
}

hipError_t launch_spmm(const aijhip_mat &A, int32_t k, int layout, const double *X, int64_t ldx, double *Y,
                       int64_t ldy, hipStream_t s, const SpmmOp &op, const int *stop) {
    if (A.m == 0) return hipSuccess;
    const int path = spmm_path(A);
    const bool il = layout == AIJHIP_DENSE_INTERLEAVED;
    if (op.op != kSpmmPlain) {  // the epilogues: interleaved blocks, the operands they name present
        const bool square = op.op == kSpmmPost || op.op == kSpmmCheby;
        if (!il || !op.B || (square && (!op.dinv || A.m != A.n || X == Y))) return hipErrorInvalidValue;
    }
    for (int32_t j0 = 0; j0 < k;) {
        const int w = spmm_chunk_width(k - j0);
        const int64_t xo = il ? (int64_t)j0 : (int64_t)j0 * ldx, yo = il ? (int64_t)j0 : (int64_t)j0 * ldy;
        hipError_t e;
        if (op.op != kSpmmPlain)
            e = launch_op(A, path, w, Dense<true>{X + xo, Y + yo, ldx, ldy}, op, yo, stop, s);
        else if (stop)
            e = il ? launch_layout<true>(A, path, w, Dense<true>{X + xo, Y + yo, ldx, ldy}, EpPlain<true>{stop}, 0, s)
                   : launch_layout<false>(A, path, w, Dense<false>{X + xo, Y + yo, ldx, ldy}, EpPlain<true>{stop}, 0, s);
        else
            e = il ? launch_layout<true>(A, path, w, Dense<true>{X + xo, Y + yo, ldx, ldy}, EpPlain<false>{nullptr}, 0,
                                         s)
                   : launch_layout<false>(A, path, w, Dense<false>{X + xo, Y + yo, ldx, ldy}, EpPlain<false>{nullptr},
                                          0, s);
        if (e != hipSuccess) return e;
        j0 += w;
    }
    return hipSuccess;
}

}  // namespace aijhip
