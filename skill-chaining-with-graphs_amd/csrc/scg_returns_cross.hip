// scg_returns_cross.hip — SPEC §29.1: row_values_cross_kernel (per row, the value under one table of the action another table
// selects, or of a given action) and its launch.
//
// A unit of its own for the reason scg_returns.hip gives: what shares a module with a kernel may change that kernel's gfx950 code,
// and here nothing can — row_values_kernel and the scans keep theirs. The entry point and its checks are in scg_kernels.hip.
#include "scg_device.hpp"
#include "../../include/scg_abi.h"
#include <cstdlib>

using namespace scg;
typedef float f4v __attribute__((ext_vector_type(4)));

#include "scg_eval.hpp"
#include "scg_wave_phases.hpp"
#include "scg_returns_cross.hpp"

static_assert(SCG_ROW_NONE >= MAX_VF, "SCG_ROW_NONE names no table");
static_assert(RV_ROWS <= 65536, "list entries are 16-bit row indices of the slab");

// row_values_kernel's shape (scg_returns.hip): scan, lists per table by wave ballots, 8-item units, one build_tables
// and one load_b per unit. What is new: the unit's tables stay in LDS and are contracted twice, straight from W_sel[k] and from
// W_val[k]: the scan, the lists and the table build are paid once per state. That is not where a unit's time goes — measured, the
// cross call costs 1.99 row_values calls and the given mode 1.00: the contraction dominates, and the second one costs
// the unit's time again. What the kernel gives is the target in one launch, with the selection in registers.
//   cross  qs = Q^sel_k(s, .): m = SPEC §5's max and a* its lowest index are formed at once (qs is not kept over the second
//          contraction), then qv = Q^val_k(s, .) and v = qv[a*], selected by a chain of constant-index compares, never recomputed
//   GIVEN  a* = act[i] (a row with act[i] >= 5 joins no list: it is a row without a table), W_val alone is contracted
// Both contractions are contract_mem<EO_TG> on the same B operand and AB factors: each has the bits of scg_q_values for its W_k.
// Which unit an item falls into, and which wave takes it, changes no operation of its sums.
template <bool GIVEN>
__global__ __launch_bounds__(RV_WAVES * 64) void row_values_cross_kernel(const RowValuesCrossArgs A) {
    __shared__ __attribute__((aligned(16))) float2 s_z1[RV_ROWS][4];              // Z_d^1 of the listed rows
    __shared__ __attribute__((aligned(16))) float s_tab[RV_WAVES][E_TAB_FLOATS];  // per wave: the tables of one unit
    __shared__ uint16_t s_list[MAX_VF][RV_ROWS];                                  // the slab's rows by table
    __shared__ int s_cnt[MAX_VF];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n16 = lane & 15, g = lane >> 4, bi = lane & 7, cp = lane >> 3;      // lane roles: scg_eval.hpp
    const int bcol = 8 * (bi >> 2) + (bi & 3);
    const int ocol_item = 4 * (n16 >> 3) + (n16 & 3);
    const bool out_lane = (g == 0) && !(n16 & 4);
    float *cdk = s_tab[wave], *abq = s_tab[wave] + 36 * 16;
    const float *ab_lane = abq + n16 * AS + 4 * g;
    const int64_t n_slabs = (A.n + RV_ROWS - 1) / RV_ROWS;
    for (int64_t slab = blockIdx.x; slab < n_slabs; slab += gridDim.x) {
        const int64_t r0 = slab * RV_ROWS;
        if (tid < MAX_VF) s_cnt[tid] = 0;
        __syncthreads();
        // -------------------------------------------------------- scan
        int t = SCG_ROW_NONE;
        if (r0 + tid < A.n) {
            const int64_t i = r0 + tid;
            const int tb = A.tab[i];
            bool has = tb < A.n_tab;
            if (GIVEN) has = has && A.act[i] < NACT;
            if (has) {
                t = tb;
                store_z1(s_z1[tid], A.x[i], A.y[i], A.vx[i], A.vy[i]);
            } else {
                A.v[i] = 0.0f;
                if (A.a) A.a[i] = 255;
                if (!GIVEN && A.vs) A.vs[i] = 0.0f;
            }
        }
#pragma unroll
        for (int k = 0; k < MAX_VF; ++k) list_append(&s_cnt[k], s_list[k], t == k, (uint16_t)tid, lane);
        __syncthreads();
        int cnt[MAX_VF], units = 0;                            // (cnt by constant indices only: it stays in registers)
#pragma unroll
        for (int k = 0; k < MAX_VF; ++k) { cnt[k] = s_cnt[k]; units += (cnt[k] + 7) >> 3; }
        // -------------------------------------------------------- units
        for (int uu = wave; uu < units; uu += RV_WAVES) {
            int k = 0, ub = uu, ck = cnt[0];
            bool on_k = false;
#pragma unroll
            for (int kk = 0; kk < MAX_VF - 1; ++kk) {
                const int nu = (cnt[kk] + 7) >> 3;
                on_k = on_k || ub < nu;
                if (!on_k) { ub -= nu; k = kk + 1; ck = cnt[kk + 1]; }
            }
            k = __builtin_amdgcn_readfirstlane(k);             // (wave-uniform: uu and the counts are)
            const int nk = ck - 8 * ub;                        // items of this unit still ahead in the list (>= 1)
            const uint16_t *lst = &s_list[k][8 * ub];
            build_tables(s_z1[lst[min(bi, nk - 1)]], cp, bcol, cdk, abq);
            wave_lds_sync();
            float B[9], q[NACT];
            load_b(cdk, n16, g, B);
            const bool writes = out_lane && ocol_item < nk;
            const int64_t i = r0 + lst[writes ? ocol_item : 0];
            float m = 0.0f;
            int best = 0;
            if (GIVEN && writes) best = A.act[i];              // (< NACT: the scan listed the row)
#pragma unroll 1                                               // (one contraction's operands in registers at a time)
            for (int side = GIVEN ? 1 : 0; side < 2; ++side) {
                contract_mem<EO_TG>((side ? A.W_val : A.W_sel) + (size_t)k * NACT * NF, B, q, n16, g, ab_lane);
                if (!GIVEN && side == 0) {
                    m = q[0];
#pragma unroll
                    for (int aa = 1; aa < NACT; ++aa) m = fmaxf(m, q[aa]);
#pragma unroll                                                 // (a row of five NaNs: m is NaN, nothing attains it, index 0)
                    for (int aa = NACT - 1; aa >= 0; --aa) best = (q[aa] == m) ? aa : best;
                }
            }
            if (writes) {
                float v = q[0];
#pragma unroll
                for (int aa = 1; aa < NACT; ++aa) v = (best == aa) ? q[aa] : v;
                A.v[i] = v;
                if (A.a) A.a[i] = (uint8_t)best;
                if (!GIVEN && A.vs) A.vs[i] = m;
            }
            wave_lds_sync();                                   // the tables are rewritten by the next unit
        }
        __syncthreads();                                       // the lists and Z_d^1 are rewritten by the next slab
    }
}

// SCG_ROW_VALUES_CROSS_BLOCKS (>= 1) caps the launch's workgroups below RV_MAX_BLOCKS: a hook for tests and measurements, as
// SCG_ROW_VALUES_BLOCKS — the results do not depend on it
hipError_t launch_row_values_cross(const RowValuesCrossArgs &A, bool given, hipStream_t s) {
    const int64_t n_slabs = (A.n + RV_ROWS - 1) / RV_ROWS;
    int64_t blocks = n_slabs < RV_MAX_BLOCKS ? n_slabs : RV_MAX_BLOCKS;
    if (const char *ov = getenv("SCG_ROW_VALUES_CROSS_BLOCKS")) {
        const int v = atoi(ov);
        if (v >= 1 && v < blocks) blocks = v;
    }
    const dim3 grid((unsigned)blocks), block(RV_WAVES * 64);
    if (given) hipLaunchKernelGGL(row_values_cross_kernel<true>, grid, block, 0, s, A);
    else hipLaunchKernelGGL(row_values_cross_kernel<false>, grid, block, 0, s, A);
    return hipGetLastError();
}
