// cg_multi.hip — KSPMatSolve [ext]: A X = B for a block of k right-hand
// sides as k independent preconditioned CG recurrences (PC none / Jacobi, or
// GAMG through the multi-column V-cycle, mg_cycle.h) advanced in lock step, so that one iteration reads the matrix once per chunk
// of columns (launch_spmm) instead of once per column. Columns never mix: each
// has its own CGState (alpha, beta, norms, reason, its) and history, and a
// column that has stopped is frozen while the others go on.
//
// The single-vector solver (cg_device.h / cg_solve.hip, unfused: p.w from
// k_dot) is the specification, and column j equals it bit for bit:
//  - launch_spmm gives the PETSc row loop's bits per column on every path;
//  - the vector kernels run on the same grid (vec_grid blocks of 256), lane t
//    of block b owns rows (b * 256 + t) + q * grid * 256 in increasing q and,
//    for each such row, all W columns of its chunk, so every column's zz, zr,
//    rr, ss and p.w are summed in k_init / k_dot / k_update's order; block_sums
//    is bsum's tree (64-lane __shfl_down, then the waves in order);
//  - the scalar steps are cg_device.h's, one 1024-lane block per column over
//    that column's contiguous partial list (reduce_parts);
//  - the element operations are the same expressions (-ffp-contract=off).
//
// Per iteration: km_aypx, launch_spmm (W = A P, W in Z's storage), km_dot,
// km_sum_dpi, km_update, km_sum_iter; km_all_done once per batch sets the flag
// the host polls and the product stops at. With GAMG (cg_solve.hip's order):
// km_update writes R and the R.R partials only, mg_vcycle_multi gives Z = M^-1 R
// for all k columns until every column has stopped, km_dots (k_dots' order) the
// Z.Z and Z.R partials, and km_all_done runs after every iteration, so that the
// V-cycles of a finished solve's last batch return at once. The work vectors R, Z/W and P are m x k interleaved with
// leading dimension k; the chunks are launch_spmm's (spmm_chunk_width).
#include "cg_multi.h"

#include <algorithm>
#include <type_traits>

namespace {

typedef double f64x2 __attribute__((ext_vector_type(2)));

// One chunk's W columns of a caller's block (the pointer already at the
// chunk's first column): interleaved or PETSc's SeqDense columns
template <bool IL>
struct Blk {
    double *p;
    int64_t ld;
};

// W adjacent doubles of one interleaved row: 16-byte accesses (V2: the address
// is 16-byte aligned, W even) or 8-byte ones
template <int W, bool V2>
__device__ __forceinline__ void ld_row(const double *p, double (&v)[W]) {
    if constexpr (V2) {
#pragma unroll
        for (int c = 0; c < W; c += 2) {
            const f64x2 q = *reinterpret_cast<const f64x2 *>(p + c);
            v[c] = q.x;
            v[c + 1] = q.y;
        }
    } else {
#pragma unroll
        for (int c = 0; c < W; ++c) v[c] = p[c];
    }
}

template <bool NT, class T>
__device__ __forceinline__ void st1(T v, T *p) {
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// Stores of the columns whose bit is set in `live` (uniform over the block): a
// pair with one live column is stored as that column alone, so a frozen
// column is never written. Non-temporal, as the single solver's vst<true>, for
// W <= 2; plain for W >= 4, where a lane's row takes two or four store
// instructions, each leaving every line it touches partly written: measured
// at 300^3 from CSR, 200 iterations, non-temporal against plain 0.303 / 0.314 s
// at k = 2, 0.531 / 0.516 s at k = 4, 1.154 / 1.034 s at k = 8
// (profiles/kspmat/stores_ab.txt).
template <int W, bool V2>
__device__ __forceinline__ void st_row(double *p, const double (&v)[W], unsigned live) {
    constexpr bool NT = W <= 2;
    if constexpr (V2) {
#pragma unroll
        for (int c = 0; c < W; c += 2) {
            const unsigned two = (live >> c) & 3u;
            if (two == 3u) {
                f64x2 q;
                q.x = v[c];
                q.y = v[c + 1];
                st1<NT>(q, reinterpret_cast<f64x2 *>(p + c));
            } else if (two == 1u) {
                st1<NT>(v[c], p + c);
            } else if (two == 2u) {
                st1<NT>(v[c + 1], p + c + 1);
            }
        }
    } else {
#pragma unroll
        for (int c = 0; c < W; ++c)
            if ((live >> c) & 1u) st1<NT>(v[c], p + c);
    }
}

template <int W, bool IL, bool V2>
__device__ __forceinline__ void ld_blk(const Blk<IL> &b, int64_t i, double (&v)[W]) {
    if constexpr (IL) {
        ld_row<W, V2>(b.p + i * b.ld, v);
    } else {
#pragma unroll
        for (int c = 0; c < W; ++c) v[c] = b.p[i + (int64_t)c * b.ld];
    }
}

template <int W, bool IL, bool V2>
__device__ __forceinline__ void st_blk(const Blk<IL> &b, int64_t i, const double (&v)[W], unsigned live) {
    if constexpr (IL) {
        st_row<W, V2>(b.p + i * b.ld, v, live);
    } else {
#pragma unroll
        for (int c = 0; c < W; ++c)
            if ((live >> c) & 1u) __builtin_nontemporal_store(v[c], b.p + i + (int64_t)c * b.ld);
    }
}

// bsum<kVecThreads> of N values at once: each value through the same 64-lane
// tree, the per-wave results summed in wave order — by lane q for value q,
// which holds the block's sum afterwards (lanes >= N: 0). One use per kernel.
template <int N>
__device__ __forceinline__ double block_sums(double (&v)[N], double *scratch) {
    static_assert(N <= kVecThreads, "one lane per value");
    constexpr int NW = kVecThreads / 64;
    const int t = threadIdx.x;
#pragma unroll
    for (int q = 0; q < N; ++q) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[q] += __shfl_down(v[q], off, 64);
        if ((t & 63) == 0) scratch[q * NW + (t >> 6)] = v[q];
    }
    __syncthreads();
    double s = 0.0;
    if (t < N) {
#pragma unroll
        for (int w = 0; w < NW; ++w) s += scratch[t * NW + w];
    }
    return s;
}

// Column c's partial list of quantity q (nb entries, contiguous; the four
// quantities of a column follow one another as in the single solver's list)
__host__ __device__ __forceinline__ double *part_of(double *part, int nb, int c, int q) {
    return part + ((int64_t)c * kNQ + q) * nb;
}

// k_init for W columns: r = b (zero guess, x = 0) or r = b - A x (ax holds
// A x), z = D^-1 r, the partials of Z.Z, Z.R, R.R and of |D^-1 b|^2 or |b|^2.
// r, z, part: at the chunk's first column. With GAMG this is PC none's pass
// (R, the R.R partials and |b|^2 as k_init's GAMG form has them); the V-cycle
// and km_dots then overwrite Z and the Z.Z, Z.R (and |M^-1 b|^2) partials.
template <int W, bool IL, bool V2>
__global__ __launch_bounds__(kVecThreads) void km_init(int64_t n, int64_t ld, Blk<IL> B, Blk<IL> X, Blk<IL> AX,
                                                       double *r, double *z, const double *__restrict__ dinv,
                                                       double *part, CGParams p) {
    __shared__ double scratch[4 * W * (kVecThreads / 64)];
    const bool jac = p.pc == AIJHIP_PC_JACOBI;
    const bool sd = jac && p.normtype != AIJHIP_KSP_NORM_UNPRECONDITIONED;
    constexpr unsigned all = (1u << W) - 1u;
    double acc[4 * W] = {};  // zz, zr, rr, ss of column c at 4 c + 0..3
    GRID_STRIDE(i, n) {
        double bv[W], rv[W], zv[W];
        ld_blk<W, IL, V2>(B, i, bv);
        if (p.guess_zero) {
#pragma unroll
            for (int c = 0; c < W; ++c) {
                rv[c] = bv[c];
                zv[c] = 0.0;
            }
            st_blk<W, IL, V2>(X, i, zv, all);  // KSPSolve: x = 0
        } else {
            ld_blk<W, IL, V2>(AX, i, rv);
#pragma unroll
            for (int c = 0; c < W; ++c) rv[c] = bv[c] + (-1.0) * rv[c];  // VecAYPX(R,-1,B)
        }
        const double di = jac ? dinv[i] : 1.0;
#pragma unroll
        for (int c = 0; c < W; ++c) {
            const double ri = rv[c], bi = bv[c];
            const double zi = jac ? di * ri : ri;
            zv[c] = zi;
            acc[4 * c + 2] += ri * ri;
            acc[4 * c + 0] += zi * zi;
            acc[4 * c + 1] += zi * ri;
            const double sb = sd ? di * bi : bi;
            acc[4 * c + 3] += sb * sb;
        }
        st_row<W, V2>(r + i * ld, rv, all);
        st_row<W, V2>(z + i * ld, zv, all);
    }
    const double s = block_sums<4 * W>(acc, scratch);
    const int t = threadIdx.x;
    if (t < 4 * W) part_of(part, gridDim.x, t >> 2, t & 3)[blockIdx.x] = s;
}

// The chunk's scalars, read once per block: which columns still run (`live`),
// and of those which are past their first iteration (`later`)
template <int W>
__device__ __forceinline__ void chunk_state(const CGState *S, double (&a)[W], double (&b)[W], unsigned &live,
                                            unsigned &later) {
    live = later = 0;
#pragma unroll
    for (int c = 0; c < W; ++c) {
        a[c] = S[c].a;
        b[c] = S[c].b;
        if (!S[c].done) {
            live |= 1u << c;
            if (S[c].i != 0) later |= 1u << c;
        }
    }
}

// k_aypx for W columns: the previous iteration's X += a P, then P = Z (a
// column's first iteration) or P = Z + b P. z, p, S: at the chunk's first column.
template <int W, bool IL, bool V2>
__global__ __launch_bounds__(kVecThreads) void km_aypx(int64_t n, int64_t ld, const double *z, double *p, Blk<IL> X,
                                                       const CGState *S) {
    double a[W], bb[W];
    unsigned live, later;
    chunk_state<W>(S, a, bb, live, later);
    if (!live) return;
    GRID_STRIDE(i, n) {
        double pv[W], zv[W];
        ld_row<W, V2>(p + i * ld, pv);
        ld_row<W, V2>(z + i * ld, zv);
        if (later) {
            double xv[W];
            ld_blk<W, IL, V2>(X, i, xv);
#pragma unroll
            for (int c = 0; c < W; ++c) xv[c] = xv[c] + a[c] * pv[c];
            st_blk<W, IL, V2>(X, i, xv, later);
        }
#pragma unroll
        for (int c = 0; c < W; ++c) pv[c] = ((later >> c) & 1u) ? zv[c] + bb[c] * pv[c] : zv[c];
        st_row<W, V2>(p + i * ld, pv, live);
    }
}

// k_dot for W columns: the partials of p . w into each live column's slot 0
template <int W, bool V2>
__global__ __launch_bounds__(kVecThreads) void km_dot(int64_t n, int64_t ld, const double *p, const double *w,
                                                      double *part, const CGState *S) {
    __shared__ double scratch[W * (kVecThreads / 64)];
    unsigned live = 0;
#pragma unroll
    for (int c = 0; c < W; ++c)
        if (!S[c].done) live |= 1u << c;
    if (!live) return;
    double acc[W] = {};
    GRID_STRIDE(i, n) {
        double pv[W], wv[W];
        ld_row<W, V2>(p + i * ld, pv);
        ld_row<W, V2>(w + i * ld, wv);
#pragma unroll
        for (int c = 0; c < W; ++c) acc[c] += pv[c] * wv[c];
    }
    const double s = block_sums<W>(acc, scratch);
    const int t = threadIdx.x;
    if (t < W && ((live >> t) & 1u)) part_of(part, gridDim.x, t, 0)[blockIdx.x] = s;
}

// k_update for W columns: R -= a W, Z = D^-1 R (W and Z share storage), the
// partials of Z.Z, Z.R, R.R into each live column's slots 0, 1, 2
template <int W, bool V2>
__global__ __launch_bounds__(kVecThreads) void km_update(int64_t n, int64_t ld, double *r, double *wz,
                                                         const double *__restrict__ dinv, double *part,
                                                         const CGState *S, int pc) {
    __shared__ double scratch[3 * W * (kVecThreads / 64)];
    double a[W], bb[W];
    unsigned live, later;
    chunk_state<W>(S, a, bb, live, later);
    if (!live) return;
    const bool jac = pc == AIJHIP_PC_JACOBI, gamg = pc == AIJHIP_PC_GAMG;
    double acc[3 * W] = {};  // zz, zr, rr of column c at 3 c + 0..2
    GRID_STRIDE(i, n) {
        double rv[W], wv[W];
        ld_row<W, V2>(r + i * ld, rv);
        ld_row<W, V2>(wz + i * ld, wv);
        const double di = jac ? dinv[i] : 1.0;
#pragma unroll
        for (int c = 0; c < W; ++c) {
            const double na = -a[c];
            const double ri = rv[c] + na * wv[c];  // VecAXPY(R, -a, W)
            const double zi = jac ? di * ri : ri;  // PCApply_Jacobi
            rv[c] = ri;
            wv[c] = zi;
            acc[3 * c + 2] += ri * ri;
            acc[3 * c + 0] += zi * zi;
            acc[3 * c + 1] += zi * ri;
        }
        st_row<W, V2>(r + i * ld, rv, live);
        if (!gamg) st_row<W, V2>(wz + i * ld, wv, live);
    }
    // GAMG (k_update's form): R and the R.R partials only; Z and the Z.Z, Z.R
    // partials follow from the V-cycle and km_dots
    const double s = block_sums<3 * W>(acc, scratch);
    const int t = threadIdx.x;
    if (t < 3 * W && ((live >> (t / 3)) & 1u) && (!gamg || t % 3 == 2))
        part_of(part, gridDim.x, t / 3, t % 3)[blockIdx.x] = s;
}

// k_dots for W columns: the partials of a.a into slot sa and of a.c into slot
// sc (sc < 0: skip) of each live column (S NULL: every column), in k_dots'
// order: the same lanes own the same rows, each quantity through bsum's tree
template <int W, bool V2>
__global__ __launch_bounds__(kVecThreads) void km_dots(int64_t n, int64_t ld, const double *a, const double *c,
                                                       double *part, int sa, int sc, const CGState *S) {
    __shared__ double scratch[2 * W * (kVecThreads / 64)];
    unsigned live = 0;
#pragma unroll
    for (int q = 0; q < W; ++q)
        if (!S || !S[q].done) live |= 1u << q;
    if (!live) return;
    double acc[2 * W] = {};  // aa, ac of column q at 2 q + 0..1
    GRID_STRIDE(i, n) {
        double av[W], cv[W];
        ld_row<W, V2>(a + i * ld, av);
        if (sc >= 0) ld_row<W, V2>(c + i * ld, cv);
#pragma unroll
        for (int q = 0; q < W; ++q) {
            acc[2 * q] += av[q] * av[q];
            if (sc >= 0) acc[2 * q + 1] += av[q] * cv[q];
        }
    }
    const double s = block_sums<2 * W>(acc, scratch);
    const int t = threadIdx.x;
    if (t < 2 * W && ((live >> (t >> 1)) & 1u) && ((t & 1) == 0 || sc >= 0))
        part_of(part, gridDim.x, t >> 1, (t & 1) ? sc : sa)[blockIdx.x] = s;
}

// A block into another layout or leading dimension (B for the V-cycle's tight
// interleaved form, PCMatApply's blocks): one lane per entry
__global__ __launch_bounds__(kVecThreads) void km_copy(int64_t m, int32_t k, const double *src, int64_t lds, int sil,
                                                       double *dst, int64_t ldd, int dil) {
    GRID_STRIDE(t, m * k) {
        const int64_t i = t / k, j = t % k;
        dst[dil ? i * ldd + j : i + j * ldd] = src[sil ? i * lds + j : i + j * lds];
    }
}

// k_final_x for W columns: the last X += a P of every column whose xpend is set
template <int W, bool IL, bool V2>
__global__ __launch_bounds__(kVecThreads) void km_final_x(int64_t n, int64_t ld, const double *p, Blk<IL> X,
                                                          const CGState *S) {
    double a[W];
    unsigned pend = 0;
#pragma unroll
    for (int c = 0; c < W; ++c) {
        a[c] = S[c].a;
        if (S[c].xpend) pend |= 1u << c;
    }
    if (!pend) return;
    GRID_STRIDE(i, n) {
        double pv[W], xv[W];
        ld_row<W, V2>(p + i * ld, pv);
        ld_blk<W, IL, V2>(X, i, xv);
#pragma unroll
        for (int c = 0; c < W; ++c) xv[c] = xv[c] + a[c] * pv[c];
        st_blk<W, IL, V2>(X, i, xv, pend);
    }
}

// The scalar steps, one 1024-lane block per column (blockIdx.x): k_sum_init /
// k_sum_dpi / k_sum_iter on column j's partial list, state and history
__global__ __launch_bounds__(kRedThreads) void km_sum_init(double *part, int nb, CGState *S, double *hist,
                                                           int32_t cap, CGParams p) {
    __shared__ double scratch[kRedThreads / 64];
    const int j = blockIdx.x;
    const double zz = reduce_parts(part_of(part, nb, j, 0), nb, scratch);
    const double zr = reduce_parts(part_of(part, nb, j, 1), nb, scratch);
    const double rr = reduce_parts(part_of(part, nb, j, 2), nb, scratch);
    const double ss = reduce_parts(part_of(part, nb, j, 3), nb, scratch);
    if (threadIdx.x != 0) return;
    step_init(zz, zr, rr, ss, S + j, hist + (int64_t)j * cap, p);
}

__global__ __launch_bounds__(kRedThreads) void km_sum_dpi(double *part, int nb, CGState *S) {
    __shared__ double scratch[kRedThreads / 64];
    const int j = blockIdx.x;
    if (S[j].done) return;
    const double v = reduce_parts(part_of(part, nb, j, 0), nb, scratch);
    if (threadIdx.x != 0) return;
    step_dpi(v, S + j);
}

__global__ __launch_bounds__(kRedThreads) void km_sum_iter(double *part, int nb, CGState *S, double *hist,
                                                           int32_t cap, CGParams p) {
    __shared__ double scratch[kRedThreads / 64];
    const int j = blockIdx.x;
    if (S[j].done) return;
    const double zz = reduce_parts(part_of(part, nb, j, 0), nb, scratch);
    const double zr = reduce_parts(part_of(part, nb, j, 1), nb, scratch);
    const double rr = reduce_parts(part_of(part, nb, j, 2), nb, scratch);
    if (threadIdx.x != 0) return;
    step_iter(zz, zr, rr, S + j, hist + (int64_t)j * cap, p);
}

// The flag the host polls: 1 once every column is done
__global__ void km_all_done(const CGState *S, int k, int *flag) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int all = 1;
    for (int j = 0; j < k; ++j) all &= S[j].done != 0;
    *flag = all;
}

// f(W, IL, V2) as integral constants for a chunk of w columns
template <class F>
void with_chunk(int w, bool il, bool v2, F &&f) {
    auto wide = [&](auto W) {
        constexpr bool pairs = decltype(W)::value >= 2;
        if (il) {
            if constexpr (pairs) {
                if (v2) return f(W, std::true_type{}, std::true_type{});
            }
            return f(W, std::true_type{}, std::false_type{});
        }
        if constexpr (pairs) {
            if (v2) return f(W, std::false_type{}, std::true_type{});
        }
        return f(W, std::false_type{}, std::false_type{});
    };
    switch (w) {
        case 8: return wide(std::integral_constant<int, 8>{});
        case 4: return wide(std::integral_constant<int, 4>{});
        case 2: return wide(std::integral_constant<int, 2>{});
        default: return wide(std::integral_constant<int, 1>{});
    }
}

// One lock-step solve in flight: what the per-chunk launches need
struct MultiRun {
    CGSolve &cg;
    CGMulti &mm;
    const aijhip_mat &A;
    int32_t k;
    bool il;
    const double *B;
    int64_t ldb;
    double *X;
    int64_t ldx;
    hipStream_t s;
    const CGMultiPC *mg;  // the GAMG V-cycle (NULL: PC none / Jacobi)

    // Z = M^-1 R on the k columns of two tight interleaved blocks
    int vcycle(const double *r, double *z, const int *stop) const {
        return aijhip::mg_vcycle_multi(*mg->lv, *mg->mb, k, r, z, s, stop);
    }
    // the partials of a.a (slot sa) and a.c (slot sc) of every live column
    void dots(const double *a, const double *c, int sa, int sc, bool masked) const {
        const int nb = mm.nb;
        chunks([&](auto W, auto, auto V2, int32_t j0) {
            constexpr int w = decltype(W)::value;
            constexpr bool v2 = decltype(V2)::value;
            hipLaunchKernelGGL((km_dots<w, v2>), dim3(nb), dim3(kVecThreads), 0, s, (int64_t)cg.m, (int64_t)k, a + j0,
                               c ? c + j0 : nullptr, part_of(mm.d_part, nb, j0, 0), sa, sc,
                               masked ? mm.d_state + j0 : nullptr);
        });
    }

    // f(W, IL, V2, j0) for every chunk of the k columns. 16-byte accesses only
    // where every address they are issued at is 16-byte aligned: the work
    // vectors (ld = k) need k even, an interleaved B and X an aligned first
    // column and even leading dimensions; column blocks are read by 8 bytes.
    template <class F>
    void chunks(F &&f) const {
        for (int32_t j0 = 0; j0 < k;) {
            const int w = aijhip::spmm_chunk_width(k - j0);
            bool v2 = w >= 2 && (k & 1) == 0;
            if (v2 && il)
                v2 = ((reinterpret_cast<uintptr_t>(B + j0) | reinterpret_cast<uintptr_t>(X + j0)) & 15) == 0 &&
                     ((ldb | ldx) & 1) == 0;
            with_chunk(w, il, v2, [&](auto W, auto IL, auto V2) { f(W, IL, V2, j0); });
            j0 += w;
        }
    }
    template <bool IL>
    Blk<IL> blk(const double *base, int64_t ld, int32_t j0) const {
        return Blk<IL>{const_cast<double *>(base) + (IL ? (int64_t)j0 : (int64_t)j0 * ld), ld};
    }
};

int multi_iteration(const MultiRun &R, const CGParams &p) {
    CGSolve &cg = R.cg;
    CGMulti &mm = R.mm;
    const int64_t m = cg.m, ld = R.k;
    const int nb = mm.nb;
    const dim3 vg(nb), vt(kVecThreads), rt(kRedThreads), kg(R.k);
    hipStream_t s = R.s;
    R.chunks([&](auto W, auto IL, auto V2, int32_t j0) {
        constexpr int w = decltype(W)::value;
        constexpr bool il = decltype(IL)::value, v2 = decltype(V2)::value;
        hipLaunchKernelGGL((km_aypx<w, il, v2>), vg, vt, 0, s, m, ld, mm.d_z + j0, mm.d_p + j0,
                           R.blk<il>(R.X, R.ldx, j0), mm.d_state + j0);
    });
    // W = A P for all columns (W shares Z's storage); frozen columns' W is never read
    const hipError_t e = aijhip::launch_spmm(R.A, R.k, AIJHIP_DENSE_INTERLEAVED, mm.d_p, ld, mm.d_z, ld, s,
                                             aijhip::SpmmOp(), mm.d_flag);
    if (e != hipSuccess) return cg_hip(e, "KSPMatSolve product");
    R.chunks([&](auto W, auto, auto V2, int32_t j0) {
        constexpr int w = decltype(W)::value;
        constexpr bool v2 = decltype(V2)::value;
        hipLaunchKernelGGL((km_dot<w, v2>), vg, vt, 0, s, m, ld, mm.d_p + j0, mm.d_z + j0,
                           part_of(mm.d_part, nb, j0, 0), mm.d_state + j0);
    });
    hipLaunchKernelGGL(km_sum_dpi, kg, rt, 0, s, mm.d_part, nb, mm.d_state);
    R.chunks([&](auto W, auto, auto V2, int32_t j0) {
        constexpr int w = decltype(W)::value;
        constexpr bool v2 = decltype(V2)::value;
        hipLaunchKernelGGL((km_update<w, v2>), vg, vt, 0, s, m, ld, mm.d_r + j0, mm.d_z + j0, cg.d_dinv,
                           part_of(mm.d_part, nb, j0, 0), mm.d_state + j0, cg.pc);
    });
    if (R.mg) {  // Z = M^-1 R on every column until all have stopped, then k_dots' Z.Z and Z.R
        if (const int rc = R.vcycle(mm.d_r, mm.d_z, mm.d_flag)) return rc;
        R.dots(mm.d_z, mm.d_r, 0, 1, true);
    }
    hipLaunchKernelGGL(km_sum_iter, kg, rt, 0, s, mm.d_part, nb, mm.d_state, mm.d_hist, mm.hist_cap, p);
    // with a V-cycle the flag is set after every iteration, so that the rest of a
    // batch costs launches only; PC none / Jacobi: once per batch (cgm_solve)
    if (R.mg) hipLaunchKernelGGL(km_all_done, dim3(1), dim3(64), 0, s, mm.d_state, R.k, mm.d_flag);
    const hipError_t e2 = hipGetLastError();
    return e2 == hipSuccess ? AIJHIP_OK : cg_hip(e2, "KSPMatSolve iteration");
}

}  // namespace

// The work vectors for k columns of m rows and histories of cg.max_it + 2 entries
int cgm_reserve(const CGSolve &cg, CGMulti &mm, int32_t k) {
    const int32_t hcap = cg.max_it + 2;
    if (mm.cap_k >= k && mm.hist_cap >= hcap && mm.m == cg.m && mm.nb == cg.vec_grid) return AIJHIP_OK;
    const int32_t cap = std::max(k, mm.cap_k);
    cgm_free(mm);
    const size_t vb = sizeof(double) * (size_t)std::max<int64_t>(cg.m, 1) * (size_t)cap;
    hipError_t e;
    if ((e = hipMalloc(&mm.d_r, vb)) != hipSuccess || (e = hipMalloc(&mm.d_z, vb)) != hipSuccess ||
        (e = hipMalloc(&mm.d_p, vb)) != hipSuccess ||
        (e = hipMalloc(&mm.d_part, sizeof(double) * (size_t)kNQ * (size_t)cg.vec_grid * (size_t)cap)) != hipSuccess ||
        (e = hipMalloc(&mm.d_hist, sizeof(double) * (size_t)hcap * (size_t)cap)) != hipSuccess ||
        (e = hipMalloc(&mm.d_state, sizeof(CGState) * (size_t)cap)) != hipSuccess ||
        (e = hipMalloc(&mm.d_flag, sizeof(int))) != hipSuccess ||
        (e = hipHostMalloc(&mm.h_state, sizeof(CGState) * (size_t)cap, hipHostMallocDefault)) != hipSuccess ||
        (e = hipHostMalloc(&mm.h_flag, sizeof(int), hipHostMallocDefault)) != hipSuccess) {
        cgm_free(mm);
        return cg_hip(e, "KSPMatSolve work vectors");
    }
    mm.cap_k = cap;
    mm.hist_cap = hcap;
    mm.m = cg.m;
    mm.nb = cg.vec_grid;
    return AIJHIP_OK;
}

void cgm_copy_block(int64_t m, int32_t k, int n_cu, const double *src, int64_t lds, bool sil, double *dst,
                    int64_t ldd, bool dil, hipStream_t s) {
    const int64_t n = m * k;
    if (n <= 0) return;
    const dim3 g((unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kVecThreads - 1) / kVecThreads,
                                                                  (int64_t)std::max(n_cu, 1) * 8)));
    hipLaunchKernelGGL(km_copy, g, dim3(kVecThreads), 0, s, m, k, src, lds, sil ? 1 : 0, dst, ldd, dil ? 1 : 0);
}

void cgm_free(CGMulti &mm) {
    hipFree(mm.d_r); hipFree(mm.d_z); hipFree(mm.d_p); hipFree(mm.d_part); hipFree(mm.d_hist);
    hipFree(mm.d_state); hipFree(mm.d_flag);
    if (mm.h_state) hipHostFree(mm.h_state);
    if (mm.h_flag) hipHostFree(mm.h_flag);
    mm.d_r = mm.d_z = mm.d_p = mm.d_part = mm.d_hist = nullptr;
    mm.d_state = mm.h_state = nullptr;
    mm.d_flag = mm.h_flag = nullptr;
    mm.cap_k = mm.hist_cap = 0;
    mm.m = 0;
    mm.nb = 0;
}

int cgm_solve(CGSolve &cg, CGMulti &mm, const aijhip_mat &A, int32_t k, int layout, const double *B, int64_t ldb,
              double *X, int64_t ldx, hipStream_t s, const CGMultiPC *mg) {
    if ((cg.pc == AIJHIP_PC_GAMG) != (mg != nullptr))
        return cg_fail(AIJHIP_ERR_STATE, "KSPMatSolve: the V-cycle goes with PC GAMG");
    int rc = cgm_reserve(cg, mm, k);
    if (rc) return rc;
    const int64_t m = cg.m, ld = k;
    const bool il = layout == AIJHIP_DENSE_INTERLEAVED;
    const CGParams p{cg.rtol, cg.abstol, cg.dtol, cg.max_it, cg.normtype, cg.guess_nonzero ? 0 : 1, cg.pc};
    const MultiRun R{cg, mm, A, k, il, B, ldb, X, ldx, s, mg};
    const int nb = mm.nb;
    const dim3 vg(nb), vt(kVecThreads), rt(kRedThreads), kg(k);
    hipError_t e = hipSuccess;
    // a column that stops at the top of or inside an iteration (indefinite PC
    // or matrix, beta = 0) logs no norm for it: that entry of its its + 1
    // reads 0, not a previous solve's norm
    if ((e = hipMemsetAsync(mm.d_hist, 0, sizeof(double) * (size_t)mm.hist_cap * (size_t)k, s)) != hipSuccess)
        return cg_hip(e, "KSPMatSolve init");
    // nonzero initial guess: A X into P's storage (free until the first
    // P = Z) in the caller's layout, from where km_init reads it
    const int64_t ldax = il ? ld : std::max<int64_t>(m, 1);
    if (cg.guess_nonzero && (e = aijhip::launch_spmm(A, k, layout, X, ldx, mm.d_p, ldax, s)) != hipSuccess)
        return cg_hip(e, "KSPMatSolve init");
    R.chunks([&](auto W, auto IL, auto V2, int32_t j0) {
        constexpr int w = decltype(W)::value;
        constexpr bool cil = decltype(IL)::value, v2 = decltype(V2)::value;
        hipLaunchKernelGGL((km_init<w, cil, v2>), vg, vt, 0, s, m, ld, R.blk<cil>(B, ldb, j0), R.blk<cil>(X, ldx, j0),
                           R.blk<cil>(mm.d_p, ldax, j0), mm.d_r + j0, mm.d_z + j0, cg.d_dinv,
                           part_of(mm.d_part, nb, j0, 0), p);
    });
    if (mg) {
        // cg_solve's order; no stop flag yet (the first scalar step initialises the states)
        if (cg.guess_nonzero && cg.normtype != AIJHIP_KSP_NORM_UNPRECONDITIONED) {
            // snorm = |M^-1 b| per column: the V-cycle on B, through the finest
            // staging block when B is not tight interleaved
            const double *bt = B;
            if (!il || ldb != ld) {
                cgm_copy_block(m, k, A.n_cu, B, ldb, il, mg->mb->lev[0].b, ld, true, s);
                bt = mg->mb->lev[0].b;
            }
            if ((rc = R.vcycle(bt, mm.d_z, nullptr))) return rc;
            R.dots(mm.d_z, nullptr, 3, -1, false);
        }
        if ((rc = R.vcycle(mm.d_r, mm.d_z, nullptr))) return rc;
        R.dots(mm.d_z, mm.d_r, 0, 1, false);
    }
    hipLaunchKernelGGL(km_sum_init, kg, rt, 0, s, mm.d_part, nb, mm.d_state, mm.d_hist, mm.hist_cap, p);
    hipLaunchKernelGGL(km_all_done, dim3(1), dim3(64), 0, s, mm.d_state, k, mm.d_flag);
    if ((e = hipGetLastError()) != hipSuccess) return cg_hip(e, "KSPMatSolve init");
    // iterations in batches between polls of the all-done flag, as cg_solve
    int32_t launched = 0;
    cg.waits = 0;
    for (;;) {
        ++cg.waits;
        if ((e = hipMemcpyAsync(mm.h_flag, mm.d_flag, sizeof(int), hipMemcpyDeviceToHost, s)) != hipSuccess ||
            (e = hipStreamSynchronize(s)) != hipSuccess)
            return cg_hip(e, "KSPMatSolve poll");
        if (*mm.h_flag || launched >= cg.max_it) break;
        const int32_t n = std::min<int32_t>(std::max<int32_t>(1, cg.poll), cg.max_it - launched);
        for (int32_t j = 0; j < n; ++j)
            if ((rc = multi_iteration(R, p))) return rc;
        hipLaunchKernelGGL(km_all_done, dim3(1), dim3(64), 0, s, mm.d_state, k, mm.d_flag);
        launched += n;
    }
    R.chunks([&](auto W, auto IL, auto V2, int32_t j0) {
        constexpr int w = decltype(W)::value;
        constexpr bool cil = decltype(IL)::value, v2 = decltype(V2)::value;
        hipLaunchKernelGGL((km_final_x<w, cil, v2>), vg, vt, 0, s, m, ld, mm.d_p + j0, R.blk<cil>(X, ldx, j0),
                           mm.d_state + j0);
    });
    if ((e = hipGetLastError()) != hipSuccess ||
        (e = hipMemcpyAsync(mm.h_state, mm.d_state, sizeof(CGState) * (size_t)k, hipMemcpyDeviceToHost, s)) !=
            hipSuccess ||
        (e = hipStreamSynchronize(s)) != hipSuccess)
        return cg_hip(e, "KSPMatSolve final update");
    ++cg.waits;
    mm.k = k;
    mm.its.assign((size_t)k, 0);
    mm.reason.assign((size_t)k, 0);
    mm.rnorm.assign((size_t)k, 0.0);
    mm.hist.assign((size_t)k, std::vector<double>());
    for (int32_t j = 0; j < k; ++j) {
        const CGState &st = mm.h_state[j];
        mm.its[j] = st.its;
        mm.reason[j] = st.reason ? st.reason : AIJHIP_KSP_DIVERGED_ITS;
        mm.rnorm[j] = st.dp;
        const int32_t nh = std::min<int32_t>(mm.hist_cap, st.its + 1);
        mm.hist[j].resize((size_t)std::max(nh, 0));
        if (nh > 0 && (e = hipMemcpy(mm.hist[j].data(), mm.d_hist + (int64_t)j * mm.hist_cap,
                                     sizeof(double) * (size_t)nh, hipMemcpyDeviceToHost)) != hipSuccess)
            return cg_hip(e, "residual history");
    }
    // what PETSc's KSPMatSolve column loop leaves in the KSP: the last column
    cg.its = mm.its[k - 1];
    cg.reason = mm.reason[k - 1];
    cg.rnorm = mm.rnorm[k - 1];
    cg.hist = mm.hist[k - 1];
    return AIJHIP_OK;
}
