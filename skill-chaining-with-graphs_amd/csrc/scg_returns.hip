// scg_returns.hip — SPEC §27: row_values_kernel (one greedy value per row under a per-row table) and lambda_returns_kernel (the
// backward scan of the lambda-return over every env's rows), SPEC §28: trace_returns_kernel (that scan with a trace coefficient per
// row), and their launches.
//
// A unit of its own for the reason scg_step_gate.hip gives: what shares a module with a kernel may change that kernel's gfx950 code,
// and here nothing can. The entry points and their checks are in scg_kernels.hip. The wave-phase header comes in for store_z1 and
// list_append, scg_eval.hpp for the E unit; no other kernel template is instantiated here.
#include "scg_device.hpp"
#include "../../include/scg_abi.h"
#include <cstdlib>

using namespace scg;
typedef float f4v __attribute__((ext_vector_type(4)));

#include "scg_eval.hpp"
#include "scg_wave_phases.hpp"
#include "scg_returns.hpp"

static_assert(SCG_ROW_NONE >= MAX_VF, "SCG_ROW_NONE names no table");
static_assert(RV_ROWS <= 65536, "list entries are 16-bit row indices of the slab");

// ------------------------------------------------------------------ SPEC §27.1
// v[i] = max_a Q_{tab[i]}(s_i, a) and the lowest a that attains it. step_gate_kernel's shape on plain rows:
//   scan   a workgroup of RV_WAVES waves owns a slab of RV_ROWS consecutive rows, one per lane: a row with a table writes Z_d^1 of its
//          state to LDS and appends itself to the list of its table (ballot / popcount: list_append); a row without one stores +0 / 255
//          and its state is never loaded
//   units  the lists in 8-item units dealt over the waves: one build_tables and one load_b per unit, then contract_mem straight from
//          W[tab] — SPEC §3.1's order, the bits of scg_q_values
//   decide SPEC §5's max (gate_holds' order) in the item's output lane, one vector store of v and one of a
// Which unit an item falls into, and which wave takes it, changes no operation of its sum: the bits do not depend on the slab, the
// list order (one atomic per wave and list: waves append in any order) or the launch geometry. Slabs are independent; a workgroup
// walks the slabs blockIdx.x, blockIdx.x + gridDim.x, ...
__global__ __launch_bounds__(RV_WAVES * 64) void row_values_kernel(const RowValuesArgs A) {
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
            if (tb < A.n_tab) {
                t = tb;
                store_z1(s_z1[tid], A.x[i], A.y[i], A.vx[i], A.vy[i]);
            } else {
                A.v[i] = 0.0f;
                if (A.a) A.a[i] = 255;
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
            contract_mem<EO_TG>(A.W + (size_t)k * NACT * NF, B, q, n16, g, ab_lane);
            if (out_lane && ocol_item < nk) {
                const int64_t i = r0 + lst[ocol_item];
                float m = q[0];
#pragma unroll
                for (int aa = 1; aa < NACT; ++aa) m = fmaxf(m, q[aa]);
                int best = 0;                                  // (a row of five NaNs: m is NaN, nothing attains it, index 0)
#pragma unroll
                for (int aa = NACT - 1; aa >= 0; --aa) best = (q[aa] == m) ? aa : best;
                A.v[i] = m;
                if (A.a) A.a[i] = (uint8_t)best;
            }
            wave_lds_sync();                                   // the tables are rewritten by the next unit
        }
        __syncthreads();                                       // the lists and Z_d^1 are rewritten by the next slab
    }
}

// SCG_ROW_VALUES_BLOCKS (>= 1) caps the launch's workgroups below RV_MAX_BLOCKS: a hook for tests and measurements, as
// SCG_STEP_GATE_ENVS — the results do not depend on it
hipError_t launch_row_values(const RowValuesArgs &A, hipStream_t s) {
    const int64_t n_slabs = (A.n + RV_ROWS - 1) / RV_ROWS;
    int64_t blocks = n_slabs < RV_MAX_BLOCKS ? n_slabs : RV_MAX_BLOCKS;
    if (const char *ov = getenv("SCG_ROW_VALUES_BLOCKS")) {
        const int v = atoi(ov);
        if (v >= 1 && v < blocks) blocks = v;
    }
    hipLaunchKernelGGL(row_values_kernel, dim3((unsigned)blocks), dim3(RV_WAVES * 64), 0, s, A);
    return hipGetLastError();
}

// ------------------------------------------------------------------ SPEC §27.2
// one lane's value from lane `src` of the wave (src wave-uniform), both halves of the binary64
__device__ __forceinline__ double lane_value(double v, int src) {
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src), lo = __builtin_amdgcn_readlane(__double2loint(v), src);
    return __hiloint2double(hi, lo);
}

// how a row forms its two values from the row behind it (the kernel's per-lane precomputation; SPEC §27.2's cases)
enum { LR0_END = 0, LR0_LAST = 1, LR0_MIX = 2 };                                  // the root stream: r / r + gamma b0 / r + gamma mix(b0, y0')
enum { LRK_NONE = 0, LRK_END = 1, LRK_FIXED = 2, LRK_ROOT = 3, LRK_OWN = 4 };     // the option stream: +0 / rb / rb + a term without y' /
                                                                                   // rb + gamma mix(b0, y0') / rb + gamma mix(bk, yk')

// One wave per env, its rows in chunks of 64 from the end: lane i of a chunk holds row base + i, loads it coalesced and precomputes what
// does not depend on the row behind ((1 - lambda) b, the fixed terms, the case). Then the chunk's dependent steps run from lane 63
// down, wave-uniformly: every lane evaluates ITS row's expressions on the carried (y0', yk') — only lane i's are meaningful at step i
// — lane i keeps them, and they are read back from lane i as the next step's carry. The carry crosses chunks in registers. Every
// operation is a binary64 __dmul_rn / __dadd_rn: rounded once, never fused.
__global__ __launch_bounds__(LR_WAVES * 64) void lambda_returns_kernel(const LambdaReturnsArgs A) {
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * LR_WAVES + (threadIdx.x >> 6);
    if (e >= A.n_env) return;                                  // (wave-uniform)
    int64_t lo = A.offsets[e], hi = A.offsets[e + 1];
    lo = lo < 0 ? 0 : (lo > A.total ? A.total : lo);           // no offsets reach outside [0, total)
    hi = hi < lo ? lo : (hi > A.total ? A.total : hi);
    const int64_t L = hi - lo;
    const double gamma = A.gamma, lam = A.lam, oml = __dadd_rn(1.0, -lam);        // 1 - lambda, formed once
    double c0n = 0.0, ckn = 0.0;                               // the carry: y0 and yk of the row behind the chunk
    for (int64_t top = L; top > 0; top -= 64) {
        const int64_t base = top - 64, j = base + lane;        // this lane's local row (< top; < 0: no row)
        int m0 = LR0_END, mk = LRK_NONE;
        double r = 0.0, rb = 0.0, fix0 = 0.0, fixk = 0.0, mb0 = 0.0, mbk = 0.0;
        if (j >= 1) {
            const int64_t i = lo + j;
            const bool last = (j == L - 1), end = A.done[i] != 0;
            const int o = A.vf[i], tm = A.term[i];
            const double b0 = (double)A.v0[i], bk = (double)A.vk[i];
            r = (double)A.reward[i];
            m0 = end ? LR0_END : (last ? LR0_LAST : LR0_MIX);
            fix0 = __dadd_rn(r, __dmul_rn(gamma, b0));         // r + gamma b0
            mb0 = __dmul_rn(oml, b0);
            if (o >= 1) {
                rb = __dadd_rn(r, tm == SCG_TRIAL_SUCCESS ? A.r_succ : 0.0);
                if (end) mk = LRK_END;
                else if (tm != 0) {
                    mk = last ? LRK_FIXED : LRK_ROOT;
                    fixk = __dadd_rn(rb, __dmul_rn(gamma, b0));
                } else {
                    const bool same = !last && (int)A.vf[i + 1] == o;
                    mk = same ? LRK_OWN : LRK_FIXED;
                    fixk = __dadd_rn(rb, __dmul_rn(gamma, bk));
                    mbk = __dmul_rn(oml, bk);
                }
            }
        }
        double y0 = 0.0, yk = 0.0;                             // (row 0, the begin row: +0 both)
        const int first = base >= 1 ? 0 : (int)(1 - base);     // the chunk's lowest lane that holds a step row
        for (int i = 63; i >= first; --i) {
            const double g0 = __dmul_rn(gamma, __dadd_rn(mb0, __dmul_rn(lam, c0n)));      // gamma mix(b0, y0')
            const double gk = __dmul_rn(gamma, __dadd_rn(mbk, __dmul_rn(lam, ckn)));      // gamma mix(bk, yk')
            const double t0 = m0 == LR0_END ? r : (m0 == LR0_LAST ? fix0 : __dadd_rn(r, g0));
            const double tk = mk == LRK_NONE ? 0.0 : mk == LRK_END ? rb : mk == LRK_FIXED ? fixk
                            : __dadd_rn(rb, mk == LRK_ROOT ? g0 : gk);
            if (lane == i) { y0 = t0; yk = tk; }
            c0n = lane_value(t0, i);
            ckn = lane_value(tk, i);
        }
        if (j >= 0) { A.y0[lo + j] = y0; A.yk[lo + j] = yk; }
    }
}

hipError_t launch_lambda_returns(const LambdaReturnsArgs &A, hipStream_t s) {
    hipLaunchKernelGGL(lambda_returns_kernel, dim3((A.n_env + LR_WAVES - 1) / LR_WAVES), dim3(LR_WAVES * 64), 0, s, A);
    return hipGetLastError();
}

// ------------------------------------------------------------------ SPEC §28.1
// lambda_returns_kernel's scan with the trace coefficient a per-row operand: a row's mix takes c = c_{j+1}, the coefficient of the
// row behind it — +0 where SCG_TRACE_CUT is set and that row's recorded action is not the greedy action `ag` of the row in front,
// else lam[vf of that row] — and omc = 1 - c, formed per row by one subtraction. c is selected, never computed. A lane reads
// action[i + 1], ag[i] and vf[i + 1] only where its row has a row behind it in its env (j < L - 1), so i + 1 < hi <= total. The
// cases, the operation sequence and the carry are lambda_returns_kernel's: with every c = lambda the bits are its bits. WITH_H adds
// the root stream's horizon h_j = 1 + c h_{j+1} as a third carry; without it nothing of h is formed. A kernel of its own, so that
// no instruction of lambda_returns_kernel moves.
template <bool WITH_H>
__global__ __launch_bounds__(LR_WAVES * 64) void trace_returns_kernel(const TraceReturnsArgs A) {
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * LR_WAVES + (threadIdx.x >> 6);
    if (e >= A.n_env) return;                                  // (wave-uniform)
    int64_t lo = A.offsets[e], hi = A.offsets[e + 1];
    lo = lo < 0 ? 0 : (lo > A.total ? A.total : lo);           // no offsets reach outside [0, total)
    hi = hi < lo ? lo : (hi > A.total ? A.total : hi);
    const int64_t L = hi - lo;
    const double gamma = A.gamma;
    const bool cut_on = (A.flags & SCG_TRACE_CUT) != 0;
    double c0n = 0.0, ckn = 0.0, chn = 0.0;                    // the carry: y0, yk and h of the row behind the chunk
    for (int64_t top = L; top > 0; top -= 64) {
        const int64_t base = top - 64, j = base + lane;        // this lane's local row (< top; < 0: no row)
        int m0 = LR0_END, mk = LRK_NONE;
        double r = 0.0, rb = 0.0, fix0 = 0.0, fixk = 0.0, mb0 = 0.0, mbk = 0.0, c = 0.0;
        if (j >= 1) {
            const int64_t i = lo + j;
            const bool last = (j == L - 1), end = A.done[i] != 0;
            const int o = A.vf[i], tm = A.term[i];
            const double b0 = (double)A.v0[i], bk = (double)A.vk[i];
            int vn = SCG_ROW_NONE;                             // vf[j + 1]; read, with the coefficient, where row j + 1 exists
            if (!last) {
                vn = A.vf[i + 1];
                const int sel = vn < A.n_lam ? vn : 0;
                double cl = A.lam[0];                          // (constant indices only: the table stays in scalar registers)
#pragma unroll
                for (int k = 1; k < MAX_VF; ++k) cl = (sel == k) ? A.lam[k] : cl;
                c = (cut_on && A.action[i + 1] != A.ag[i]) ? 0.0 : cl;
            }
            const double omc = __dadd_rn(1.0, -c);             // 1 - c, per row
            r = (double)A.reward[i];
            m0 = end ? LR0_END : (last ? LR0_LAST : LR0_MIX);
            fix0 = __dadd_rn(r, __dmul_rn(gamma, b0));         // r + gamma b0
            mb0 = __dmul_rn(omc, b0);
            if (o >= 1) {
                rb = __dadd_rn(r, tm == SCG_TRIAL_SUCCESS ? A.r_succ : 0.0);
                if (end) mk = LRK_END;
                else if (tm != 0) {
                    mk = last ? LRK_FIXED : LRK_ROOT;
                    fixk = __dadd_rn(rb, __dmul_rn(gamma, b0));
                } else {
                    const bool same = !last && vn == o;
                    mk = same ? LRK_OWN : LRK_FIXED;
                    fixk = __dadd_rn(rb, __dmul_rn(gamma, bk));
                    mbk = __dmul_rn(omc, bk);
                }
            }
        }
        double y0 = 0.0, yk = 0.0, h = 0.0;                    // (row 0, the begin row: +0 all)
        const int first = base >= 1 ? 0 : (int)(1 - base);     // the chunk's lowest lane that holds a step row
        for (int i = 63; i >= first; --i) {
            const double g0 = __dmul_rn(gamma, __dadd_rn(mb0, __dmul_rn(c, c0n)));        // gamma mix(b0, y0')
            const double gk = __dmul_rn(gamma, __dadd_rn(mbk, __dmul_rn(c, ckn)));        // gamma mix(bk, yk')
            const double t0 = m0 == LR0_END ? r : (m0 == LR0_LAST ? fix0 : __dadd_rn(r, g0));
            const double tk = mk == LRK_NONE ? 0.0 : mk == LRK_END ? rb : mk == LRK_FIXED ? fixk
                            : __dadd_rn(rb, mk == LRK_ROOT ? g0 : gk);
            if (lane == i) { y0 = t0; yk = tk; }
            c0n = lane_value(t0, i);
            ckn = lane_value(tk, i);
            if (WITH_H) {
                const double th = m0 == LR0_MIX ? __dadd_rn(1.0, __dmul_rn(c, chn)) : 1.0;
                if (lane == i) h = th;
                chn = lane_value(th, i);
            }
        }
        if (j >= 0) {
            A.y0[lo + j] = y0; A.yk[lo + j] = yk;
            if (WITH_H) A.h[lo + j] = h;
        }
    }
}

hipError_t launch_trace_returns(const TraceReturnsArgs &A, hipStream_t s) {
    const dim3 grid((A.n_env + LR_WAVES - 1) / LR_WAVES), block(LR_WAVES * 64);
    if (A.h) hipLaunchKernelGGL(trace_returns_kernel<true>, grid, block, 0, s, A);
    else hipLaunchKernelGGL(trace_returns_kernel<false>, grid, block, 0, s, A);
    return hipGetLastError();
}
