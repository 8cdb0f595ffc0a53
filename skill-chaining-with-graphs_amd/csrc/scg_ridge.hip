// scg_ridge.hip — SPEC §31: the pinned-order ridge solve, a batched binary64 Cholesky factor-and-solve (ridge_factor_kernel, one
// launch per block column, and ridge_subst_kernel) and their launch.
//
// A unit of its own for the reason scg_returns.hip gives: what shares a module with a kernel may change that kernel's gfx950 code,
// and here nothing can. The entry point and its checks are in scg_kernels.hip.
//
// The contract is one binary64 operation at a time (the Makefile's -ffp-contract=off: a product and the difference that takes it
// are two roundings), every entry's updates in ascending k. Left-looking by block columns of 16 keeps that order: the launch of block
// column J applies, to each entry of the column, the finished columns k < 16 J in ascending k, then the columns of its own diagonal
// tile one by one. Block columns depend on each other through launch boundaries only: no workgroup waits on another.
#include "scg_ridge.hpp"
#include "../../include/scg_abi.h"

static_assert(RIDGE_KCHUNK % RIDGE_TILE == 0, "a chunk is whole tiles");
static_assert(RIDGE_MAX_F == SCG_RIDGE_MAX_F && RIDGE_MAX_MAT == SCG_GRAM_MAX_SEGMENTS, "the header's limits are the kernels'");

// One workgroup = one tile (I, J), I >= J, of one matrix: 256 threads, thread (r, c) owns entry (16 I + r, 16 J + c) and, for the
// diagonal tile every workgroup of the column recomputes (twice the arithmetic, no hand-off), entry (16 J + r, 16 J + c). Rows I
// and J of the finished part of L pass through LDS in chunks of RIDGE_KCHUNK columns, k-major so that a wave's reads fall in
// consecutive words. The first read of M folds in the conversion from binary32 and the diagonal's mu * lam. The workgroup I = J
// stores the diagonal tile and, on a failed pivot, info; the others store their own tile. A matrix whose info is set, here or by an
// earlier launch, is left alone: every workgroup of the column finds the same failed pivot by the same operations.
__global__ __launch_bounds__(RIDGE_TILE * RIDGE_TILE) void ridge_factor_kernel(const RidgeArgs P) {
    __shared__ double s_i[RIDGE_KCHUNK][RIDGE_TILE + 1], s_j[RIDGE_KCHUNK][RIDGE_TILE + 1];
    __shared__ double s_d[RIDGE_TILE][RIDGE_TILE + 1], s_e[RIDGE_TILE][RIDGE_TILE + 1];
    __shared__ int s_fail, s_stop;
    const int g = blockIdx.y, J = P.J, I = J + (int)blockIdx.x;
    if ((P.skip >> g) & 1) return;
    const int tid = threadIdx.x, r = tid >> 4, c = tid & 15;
    if (tid == 0) { s_stop = P.info[g]; s_fail = 0; }            // (one read for the workgroup: the column's workgroup I = J may set
    __syncthreads();                                            //  info while the others start, and a barrier follows)
    if (s_stop != 0) return;
    const size_t F = (size_t)P.F;
    const bool diag = I == J;
    const float *Ag = P.A + (size_t)g * F * F;
    double *Lg = P.work + (size_t)g * F * F;
    const size_t row_i = (size_t)RIDGE_TILE * I + r, row_j = (size_t)RIDGE_TILE * J + r, col = (size_t)RIDGE_TILE * J + c;
    double acc_i = 0.0, acc_j = 0.0;
    if (!diag) acc_i = (double)Ag[row_i * F + col];
    if (r >= c) {                                               // (the strict upper triangle of A is never read)
        acc_j = (double)Ag[row_j * F + col];
        if (r == c) acc_j = acc_j + P.mu[g] * P.lam[col];
    }
    // -------------------------------------------------------- the finished columns k < 16 J, ascending
    const int K = RIDGE_TILE * J;
    for (int k0 = 0; k0 < K; k0 += RIDGE_KCHUNK) {
        const int kn = K - k0 < RIDGE_KCHUNK ? K - k0 : RIDGE_KCHUNK;
        __syncthreads();
#pragma unroll
        for (int m = 0; m < RIDGE_KCHUNK / RIDGE_TILE; ++m) {
            const int kk = c + RIDGE_TILE * m;
            if (kk < kn) {
                s_j[kk][r] = Lg[row_j * F + k0 + kk];
                if (!diag) s_i[kk][r] = Lg[row_i * F + k0 + kk];
            }
        }
        __syncthreads();
        for (int kb = 0; kb < kn; kb += RIDGE_TILE) {
#pragma unroll
            for (int kk = 0; kk < RIDGE_TILE; ++kk) {
                const double a = s_j[kb + kk][c];
                acc_j = acc_j - s_j[kb + kk][r] * a;
                if (!diag) acc_i = acc_i - s_i[kb + kk][r] * a;
            }
        }
    }
    // -------------------------------------------------------- the diagonal tile's own columns, one by one
    for (int jj = 0; jj < RIDGE_TILE; ++jj) {
        if (r == jj && c == jj) {
            if (!(acc_j > 0.0)) s_fail = jj + 1;
            else { acc_j = sqrt(acc_j); s_d[jj][jj] = acc_j; }
        }
        __syncthreads();
        if (s_fail) break;                                      // (uniform: written before the barrier, next written after the one below)
        const double d = s_d[jj][jj];
        if (c == jj && r > jj) { acc_j = acc_j / d; s_d[r][jj] = acc_j; }
        if (!diag && c == jj) { acc_i = acc_i / d; s_e[r][jj] = acc_i; }
        __syncthreads();
        if (c > jj && r >= c) acc_j = acc_j - s_d[r][jj] * s_d[c][jj];
        if (!diag && c > jj) acc_i = acc_i - s_e[r][jj] * s_d[c][jj];
    }
    if (s_fail) {
        if (diag && tid == 0) P.info[g] = K + s_fail;
        return;
    }
    if (diag) {
        if (r >= c) Lg[row_j * F + col] = acc_j;
    } else {
        Lg[row_i * F + col] = acc_i;
    }
}

// One workgroup = one (matrix, right-hand side): the right-hand side lives in LDS, block by block the 16 rows of the diagonal tile
// are solved serially in wave 0 (lane l holds row l; the solved entry goes round by a lane read) and the block's columns of L are
// then applied to the rows below (forward, ascending) or above (backward, descending) by all threads, a row each. A skipped or
// failed matrix gets +0.
__global__ __launch_bounds__(256) void ridge_subst_kernel(const RidgeArgs P) {
    __shared__ double s_t[RIDGE_MAX_F];
    __shared__ double s_z[RIDGE_TILE];
    const int g = blockIdx.y, q = blockIdx.x, tid = threadIdx.x, l = tid & 15;
    const int F = P.F, T = F / RIDGE_TILE;
    const size_t Fs = (size_t)F;
    double *out = P.Delta + ((size_t)g * P.n_rhs + q) * Fs;
    if (((P.skip >> g) & 1) || P.info[g] != 0) {
        for (int i = tid; i < F; i += 256) out[i] = 0.0;
        return;
    }
    const float *b = P.B + ((size_t)g * P.n_rhs + q) * Fs;
    const double *Lg = P.work + (size_t)g * Fs * Fs;
    for (int i = tid; i < F; i += 256) s_t[i] = (double)b[i];
    __syncthreads();
    // -------------------------------------------------------- forward: z_i = (b_i - sum_{k < i, ascending} L_ik z_k) / L_ii
    for (int Jb = 0; Jb < T; ++Jb) {
        const int base = RIDGE_TILE * Jb;
        if (tid < 64) {
            const double *Lr = Lg + (size_t)(base + l) * Fs + base;
            double lr[RIDGE_TILE];
#pragma unroll
            for (int jj = 0; jj < RIDGE_TILE; ++jj) lr[jj] = jj <= l ? Lr[jj] : 1.0;      // (the tile's upper triangle is not read)
            double t = s_t[base + l], z = 0.0;
#pragma unroll
            for (int jj = 0; jj < RIDGE_TILE; ++jj) {
                const double zj = __shfl(t / lr[jj], jj, 64);
                if (l == jj) z = zj;
                if (l > jj) t = t - lr[jj] * zj;
            }
            if (tid < RIDGE_TILE) { s_z[l] = z; s_t[base + l] = z; }
        }
        __syncthreads();
        for (int i = base + RIDGE_TILE + tid; i < F; i += 256) {
            const double *Lp = Lg + (size_t)i * Fs + base;
            double t = s_t[i];
#pragma unroll
            for (int jj = 0; jj < RIDGE_TILE; ++jj) t = t - Lp[jj] * s_z[jj];
            s_t[i] = t;
        }
        __syncthreads();
    }
    // -------------------------------------------------------- backward: x_i = (z_i - sum_{k > i, descending} L_ki x_k) / L_ii
    for (int Jb = T - 1; Jb >= 0; --Jb) {
        const int base = RIDGE_TILE * Jb;
        if (tid < 64) {
            const double *Lc = Lg + (size_t)base * Fs + base + l;
            double lc[RIDGE_TILE];
#pragma unroll
            for (int jj = 0; jj < RIDGE_TILE; ++jj) lc[jj] = jj >= l ? Lc[(size_t)jj * Fs] : 1.0;
            double t = s_t[base + l], x = 0.0;
#pragma unroll
            for (int jj = RIDGE_TILE - 1; jj >= 0; --jj) {
                const double xj = __shfl(t / lc[jj], jj, 64);
                if (l == jj) x = xj;
                if (l < jj) t = t - lc[jj] * xj;
            }
            if (tid < RIDGE_TILE) { s_z[l] = x; s_t[base + l] = x; }
        }
        __syncthreads();
        for (int i = tid; i < base; i += 256) {
            const double *Lp = Lg + (size_t)base * Fs + i;
            double t = s_t[i];
#pragma unroll
            for (int jj = RIDGE_TILE - 1; jj >= 0; --jj) t = t - Lp[(size_t)jj * Fs] * s_z[jj];
            s_t[i] = t;
        }
        __syncthreads();
    }
    for (int i = tid; i < F; i += 256) out[i] = s_t[i];
}

// info is zeroed, then F / 16 factor launches in block-column order and one substitution launch, all on `s`: the stream's order is
// the only dependency between them.
hipError_t launch_ridge_solve(RidgeArgs &A, hipStream_t s) {
    hipError_t e = hipMemsetAsync(A.info, 0, (size_t)A.n_mat * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    const int T = A.F / RIDGE_TILE;
    const bool any = (~A.skip & (A.n_mat >= 64 ? ~0ull : ((1ull << A.n_mat) - 1))) != 0;
    for (int J = 0; any && J < T; ++J) {
        A.J = J;
        hipLaunchKernelGGL(ridge_factor_kernel, dim3((unsigned)(T - J), (unsigned)A.n_mat), dim3(RIDGE_TILE * RIDGE_TILE), 0, s, A);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(ridge_subst_kernel, dim3((unsigned)A.n_rhs, (unsigned)A.n_mat), dim3(256), 0, s, A);
    return hipGetLastError();
}
