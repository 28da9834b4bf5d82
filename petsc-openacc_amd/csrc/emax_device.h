// emax_device.h — the vector kernels of the GAMG set-up's emax(D^-1 A)
// estimators (gamg_setup.cpp estimate_emax / estimate_emax_cg), shared by
// the single-GPU set-up (gamg_device.hip, off = 0) and the distributed one
// (gamg_mpi.hip, off = this rank's first global row: the start vector is the
// single-GPU one taken at global indices). Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// entry off + i of the start vector, uniform in [-1, 1)
__device__ __forceinline__ double emax_start(int64_t off, int32_t i) {
    return 2.0 * ((double)(mix64(0x5EEDULL + (uint64_t)(off + i + 1) * 0x9E3779B97F4A7C15ULL) >> 11) *
                  (1.0 / 9007199254740992.0)) - 1.0;
}

// the power iteration's start
__global__ void k_power_start(int32_t m, int64_t off, double *v) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) v[i] = emax_start(off, i);
}

__global__ void k_div(int32_t m, const double *w, double nw, double *v) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) v[i] = w[i] / nw;
}

// CG's estimate: the start b, r = b, z = D^-1 r, p = z; r -= a w with
// z = D^-1 r; p = z + b p
__global__ void k_cgest_start(int32_t m, int64_t off, const double *__restrict__ dinv, double *r, double *z,
                              double *p) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const double v = emax_start(off, i);
    r[i] = v;
    z[i] = dinv[i] * v;
    p[i] = z[i];
}

__global__ void k_cgest_update(int32_t m, double a, const double *__restrict__ w, const double *__restrict__ dinv,
                               double *r, double *z) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const double ri = r[i] - a * w[i];
    r[i] = ri;
    z[i] = dinv[i] * ri;
}

__global__ void k_cgest_dir(int32_t m, double b, const double *__restrict__ z, double *p) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) p[i] = z[i] + b * p[i];
}

}  // namespace
