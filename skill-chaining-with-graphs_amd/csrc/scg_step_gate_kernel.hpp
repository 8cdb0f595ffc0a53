// scg_step_gate_kernel.hpp — step_gate_kernel: SPEC §26's gate table on the step-batch (compiled in scg_step_gate.hip; scg_kernels.hip
// includes this header for the arguments and the launch's declaration only — the kernel is a template, so it has no code there).
//
// One launch between td_kernel<MODE_FUSED> and the reduce launch, only when scg_step_gated has a non-zero gate_mask. td_kernel has left,
// at every ENTERING env's position, s_next (line word [0]), the bits (on = cand, opt_steps_next == 0), both candidate qcache rows under
// the launch's W (Q_cand in the line, Q_0 in qalt) and the mark (OREC_DECLINED where its own gate() declined, else 0); commit_row has
// not read any of it yet. This kernel re-decides the entering envs whose cand is in the mask:
//   scan   a workgroup of SG_WAVES waves owns ENVS consecutive positions (64, 128 or 256: the launch's pick, results do not depend on
//          it), one per lane of its first ENVS / 64 waves: the bits, and for an entering env in the mask Z_d^1 of s_next into LDS
//          and its index into the list of its cand (ballot / popcount: list_append). About one position in ten is an offer and a
//          workgroup's units are dealt over all of its waves: a short range leaves each wave a unit or so behind the scan (small
//          env counts: latency), a long one fills the 8-item units (large env counts: throughput). DESIGN §3.31
//   units  the lists in 8-item units over the waves, as rollout_kernel's GATE instantiation walks its gate lists: ONE
//          build_tables and one load_b per unit, then contract_mem twice, option side and root side, straight from the table
//   decide gate_holds (SPEC §5's max order, a NaN side declines) in the item's output lane; where the result differs from the mark the
//          lane rewrites the mark (a vector store) and moves the env's count in hist_next between key cand and key 0 — gate()'s move,
//          in either direction. hist_next counts are integers: the order of the atomics does not matter.
// The table is only read; no workgroup waits for another; a voided step (fail_flag) is left alone.
#pragma once

constexpr int SG_WAVES = 4;                    // waves per workgroup = table areas in LDS
constexpr int SG_MIN_ENVS = 64, SG_MAX_ENVS = SG_WAVES * 64;      // positions per workgroup: a launch parameter (64, 128 or 256)

struct StepGateArgs {
    float4 *outrec;                // [positions][OREC] td_kernel's result lines: word [3].y (the mark) is rewritten where the decision flips
    const int32_t *perm;           // position -> env (never null behind scg_step's sort)
    int32_t *hist_next;            // [rows of 256 envs][8] the next order's key counts (null: the step does not fold the sort)
    const float *gate;             // [n_vf][2][5][1296], SPEC §25's layout (row 0 never read)
    const int32_t *fail_flag;      // td_kernel gave up: the step is void
    int32_t n, n_vf;
    uint32_t mask;                 // bit k: option k's offers compare the table
};

hipError_t launch_step_gate(const StepGateArgs &A, int envs, hipStream_t s);      // envs: positions per workgroup, 64 / 128 / 256

template <int NW, int ENVS>
__global__ __launch_bounds__(NW * 64) void step_gate_kernel(const StepGateArgs A) {
    static_assert(ENVS % 64 == 0 && ENVS <= NW * 64, "whole waves scan, one position per lane");
    __shared__ __attribute__((aligned(16))) float2 s_z1[ENVS][4];                 // Z_d^1 of s_next of the listed envs
    __shared__ __attribute__((aligned(16))) float s_tab[NW][E_TAB_FLOATS];        // per wave: the tables of one unit
    __shared__ uint16_t s_glist[MAX_VF][ENVS];                                    // the entering envs by cand (both sides share a list)
    __shared__ int s_gcnt[MAX_VF];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p0 = blockIdx.x * ENVS;
    if (*A.fail_flag) return;                                  // (uniform over the launch: td_kernel has finished)
    if (tid < MAX_VF) s_gcnt[tid] = 0;
    __syncthreads();
    // ------------------------------------------------------------ scan
    int cand = 0;
    if (tid < ENVS && p0 + tid < A.n) {
        const float4 *rec = A.outrec + (size_t)(p0 + tid) * OREC;
        const float4 rb = rec[1];
        const int on = (int)((__float_as_uint(rb.y) >> 16) & 255u);
        if (on >= 1 && on < A.n_vf && __float_as_int(rb.z) == 0 && ((A.mask >> on) & 1u)) {      // entering: on = cand, the option was not kept
            cand = on;
            const float4 sn = rec[0];
            store_z1(s_z1[tid], sn.x, sn.y, sn.z, sn.w);
        }
    }
    if (tid < ENVS) {                                          // (wave-uniform: whole waves scan)
#pragma unroll
        for (int k = 1; k < MAX_VF; ++k) list_append(&s_gcnt[k], s_glist[k], cand == k, (uint16_t)tid, lane);
    }
    __syncthreads();
    int gcnt[MAX_VF], gunits = 0;                              // (gcnt by constant indices only: it stays in registers)
    gcnt[0] = 0;
#pragma unroll
    for (int k = 1; k < MAX_VF; ++k) { gcnt[k] = s_gcnt[k]; gunits += (gcnt[k] + 7) >> 3; }
    // ------------------------------------------------------------ units
    const int n16 = lane & 15, g = lane >> 4, bi = lane & 7, cp = lane >> 3;      // lane roles: scg_eval.hpp
    const int bcol = 8 * (bi >> 2) + (bi & 3);
    const int ocol_item = 4 * (n16 >> 3) + (n16 & 3);
    const bool out_lane = (g == 0) && !(n16 & 4);
    float *cdk = s_tab[wave], *abq = s_tab[wave] + 36 * 16;
    const float *ab_lane = abq + n16 * AS + 4 * g;
    for (int uu = wave; uu < gunits; uu += NW) {
        int k = 1, ub = uu, ck = gcnt[1];
        bool on_k = false;
#pragma unroll
        for (int kk = 1; kk < MAX_VF - 1; ++kk) {
            const int nu = (gcnt[kk] + 7) >> 3;
            on_k = on_k || ub < nu;
            if (!on_k) { ub -= nu; k = kk + 1; ck = gcnt[kk + 1]; }
        }
        const int nk = ck - 8 * ub;                            // items of this unit still ahead in the list (>= 1)
        const uint16_t *lst = &s_glist[k][8 * ub];
        build_tables(s_z1[lst[min(bi, nk - 1)]], cp, bcol, cdk, abq);
        wave_lds_sync();
        float B[9], q[NACT], gk[NACT];
        load_b(cdk, n16, g, B);
#pragma unroll 1
        for (int side = 0; side < 2; ++side) {
            contract_mem<EO_TG>(A.gate + ((size_t)k * 2 + side) * NACT * NF, B, q, n16, g, ab_lane);
            if (side == 0) {
#pragma unroll
                for (int aa = 0; aa < NACT; ++aa) gk[aa] = q[aa];
            }
        }
        if (out_lane && ocol_item < nk) {
            const int pos = p0 + lst[ocol_item];
            const bool declined = !gate_holds(gk, q);          // SPEC §26.1: the option side against the root side
            float *mark = reinterpret_cast<float *>(A.outrec + (size_t)pos * OREC + 3) + 1;
            const bool was = __float_as_uint(*mark) == OREC_DECLINED;
            if (was != declined) {
                *mark = __uint_as_float(declined ? OREC_DECLINED : 0u);
                if (A.hist_next) {
                    const int e = A.perm ? A.perm[pos] : pos;
                    atomicAdd(&A.hist_next[(e >> 8) * 8 + k], declined ? -1 : 1);
                    atomicAdd(&A.hist_next[(e >> 8) * 8], declined ? 1 : -1);
                }
            }
        }
        wave_lds_sync();                                       // the tables are rewritten by the next unit
    }
}
