// scg_returns_cross.hpp — SPEC §29.1: the arguments and the launch of row_values_cross_kernel (compiled in scg_returns_cross.hip;
// scg_kernels.hip includes this header for the entry point's wrapper and holds no code of the kernel). The slab geometry (RV_WAVES,
// RV_ROWS, RV_MAX_BLOCKS) is scg_returns.hpp's.
#pragma once

#include "scg_returns.hpp"

struct RowValuesCrossArgs {
    const float *x, *y, *vx, *vy;  // [n] the rows' states
    const uint8_t *tab;            // [n] the row's table; SCG_ROW_NONE and every value >= n_tab: no table, the state is not read
    const float *W_sel, *W_val;    // [n_tab][5][1296] each; W_sel is not read in the given mode
    const uint8_t *act;            // [n] the given mode's selecting action (>= 5: a row without a table); null in the cross mode
    float *v;                      // [n] Q^val_tab(s, a*), +0 without a table
    uint8_t *a;                    // [n] a*, 255 without a table (null: not written)
    float *vs;                     // [n] max_a Q^sel_tab(s, a), +0 without a table (null: not written; always null in the given mode)
    int64_t n;
    int32_t n_tab;                 // 1 .. MAX_VF
};

hipError_t launch_row_values_cross(const RowValuesCrossArgs &A, bool given, hipStream_t s);      // A.n >= 1
