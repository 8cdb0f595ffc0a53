// scg_returns.hpp — SPEC §27: the arguments and the launches of row_values_kernel and lambda_returns_kernel (both compiled in
// scg_returns.hip; scg_kernels.hip includes this header for the two entry points' wrappers and holds no code of either kernel).
#pragma once

constexpr int RV_WAVES = 4;                    // waves per workgroup = table areas in LDS
constexpr int RV_ROWS = RV_WAVES * 64;         // rows of one slab: one per lane of the scan
constexpr int RV_MAX_BLOCKS = 1 << 20;         // workgroups of a launch at most; each walks the slabs blockIdx.x, + gridDim.x, ...

struct RowValuesArgs {
    const float *x, *y, *vx, *vy;  // [n] the rows' states
    const uint8_t *tab;            // [n] the row's table; SCG_ROW_NONE and every value >= n_tab: no table, the state is not read
    const float *W;                // [n_tab][5][1296]
    float *v;                      // [n] max_a Q_tab(s, a), +0 without a table
    uint8_t *a;                    // [n] the lowest index that attains it, 255 without a table (null: not written)
    int64_t n;
    int32_t n_tab;                 // 1 .. MAX_VF
};

constexpr int LR_WAVES = 4;                    // envs per workgroup: one wave walks one env's rows

struct LambdaReturnsArgs {
    const int64_t *offsets;        // [n_env + 1] env e owns rows offsets[e] .. offsets[e + 1] - 1 (clamped into [0, total] by the kernel)
    const float *reward;           // [total]
    const uint8_t *done, *vf, *term;
    const float *v0, *vk;          // [total] the bootstrap values: the root's and the row's option's at the row's state
    double *y0, *yk;               // [total] the two streams of SPEC §27.2
    double gamma, lam, r_succ;
    int64_t total;
    int32_t n_env;
};

hipError_t launch_row_values(const RowValuesArgs &A, hipStream_t s);             // A.n >= 1
hipError_t launch_lambda_returns(const LambdaReturnsArgs &A, hipStream_t s);     // A.n_env >= 1
