// scg_returns.hpp — SPEC §27, §28: the arguments and the launches of row_values_kernel, lambda_returns_kernel and trace_returns_kernel
// (all compiled in scg_returns.hip; scg_kernels.hip includes this header for the entry points' wrappers and holds no code of the kernels).
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

// SPEC §28.1: the scan with a trace coefficient per row. lambda_returns_kernel's records plus the recorded action and the greedy
// action of the table that acts on the next row; the coefficients by value function travel in the argument struct.
struct TraceReturnsArgs {
    const int64_t *offsets;        // [n_env + 1], clamped as LambdaReturnsArgs'
    const float *reward;           // [total]
    const uint8_t *done, *vf, *term;
    const uint8_t *action, *ag;    // [total] row i's recorded action; the greedy action at row i's state of the table acting on row i + 1
    const float *v0, *vk;          // [total]
    double *y0, *yk, *h;           // [total] the two streams and the root stream's horizon (h null: neither formed nor stored)
    double gamma, r_succ;
    double lam[scg::MAX_VF];       // lam[k]: the coefficient a row of value function k carries; vf >= n_lam reads lam[0]
    int64_t total;
    int32_t n_env, n_lam;          // n_lam in 1 .. MAX_VF
    uint32_t flags;                // SCG_TRACE_CUT
};

hipError_t launch_row_values(const RowValuesArgs &A, hipStream_t s);             // A.n >= 1
hipError_t launch_lambda_returns(const LambdaReturnsArgs &A, hipStream_t s);     // A.n_env >= 1
hipError_t launch_trace_returns(const TraceReturnsArgs &A, hipStream_t s);       // A.n_env >= 1
