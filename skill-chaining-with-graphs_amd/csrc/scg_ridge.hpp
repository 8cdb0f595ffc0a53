// scg_ridge.hpp — SPEC §31: the arguments and the launch of the pinned-order ridge solve (compiled in scg_ridge.hip; scg_kernels.hip
// includes this header for the entry point's wrapper and holds no code of the kernels).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

constexpr int RIDGE_TILE = 16;        // the side of a tile of L: a workgroup of 256 threads owns one, an entry per thread
constexpr int RIDGE_KCHUNK = 64;      // finished columns staged through LDS at a time (a multiple of RIDGE_TILE)
constexpr int RIDGE_MAX_F = 4096;     // SCG_RIDGE_MAX_F: the substitution keeps one right-hand side in LDS
constexpr int RIDGE_MAX_MAT = 64;     // SCG_GRAM_MAX_SEGMENTS

struct RidgeArgs {
    const float *A;                   // [n_mat][F][F], i >= j read
    const float *B;                   // [n_mat][n_rhs][F]
    const double *lam;                // [F]
    double *work;                     // [n_mat][F][F]: L in the lower triangle
    double *Delta;                    // [n_mat][n_rhs][F]
    int32_t *info;                    // [n_mat], zeroed before the first launch
    double mu[RIDGE_MAX_MAT];         // the host's scalars, by value
    uint64_t skip;                    // bit g: matrix g is skipped
    int32_t F, n_mat, n_rhs;
    int32_t J;                        // the factor launch's block column
};

hipError_t launch_ridge_solve(RidgeArgs &A, hipStream_t s);
