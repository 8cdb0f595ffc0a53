// scg_trial_kernel.hpp — trial_kernel: option trials (SPEC §9) in ONE launch (included by scg_kernels.hip, after
// scg_rollout_kernel.hpp; the geometry and the phases it shares with rollout_kernel are scg_wave_phases.hpp's).
//
// Entry i runs option k = option[i] from s0 = (x, y, vx, vy)[i] until the option terminates. With the weights frozen no trial
// reads another one's result, so a workgroup owns RO_WAVES * epw consecutive entries for the whole launch, as rollout_kernel
// does: no grid barrier, no polling, no atomics outside LDS. Per step:
//   E  Q_k(s, .) of every live entry, from the per-VF lists of the step before (the entry pass: Q_k(s0, .)) dealt in 8-item units
//      over the waves (scg_eval.hpp's E unit, W_k straight from memory: there is one value per live entry and never the root's)
//   G  qcache; after the entry pass v0 = max_a Q_k(s0, a)
//   P  each wave, one lane per entry (lanes < epw): act from qcache, Pinball physics (pinball_wave_*), SPEC §1.4's done and
//      §4.2's termination for o = k; an entry whose option goes on puts Z_d^1 of s' into its VF's list, a finished one leaves
// State, qcache and the five accumulators stay in registers; every output is written once at the end. A workgroup whose trials
// have all ended leaves the loop.
#pragma once

struct TrialArgs {
    const float *x, *y, *vx, *vy;
    const int32_t *option;
    scg_trial_out out;             // device pointers, outcome required, any other may be null
    const float *W;                // [n_vf][5][1296]
    const float *clf;              // [n_vf][8]
    const float *edges;
    const uint64_t *cellmask;
    const float *starts;           // (set by fill_shared; a trial never resets)
    int32_t n, n_vf, epw;
    uint32_t enabled, gest, parents;
    uint64_t t0, seed;
    int64_t env_base;
    float epsilon, gamma, r_succ;
    int32_t max_ep, max_opt;
    uint32_t reoffer_mask;         // (set by fill_shared; a trial never re-offers)
    MapScalars ms;
};
struct TrialRecArgs : TrialArgs {  // the recording instantiation's arguments (SPEC §10)
    scg_record rec;
};

// <false, TrialArgs>: scg_option_trials' kernel. <true, TrialRecArgs>: the same trials plus SPEC §10's rows of the entries in the
// record's window
template <bool REC, typename Args>
__global__ __launch_bounds__(RO_THREADS) void trial_kernel(const Args A) {
    __shared__ __attribute__((aligned(16))) float s_edges[MAX_EDGES * 8];
    __shared__ __attribute__((aligned(16))) float s_wave[RO_WAVES][RO_WAVE_FLOATS];
    __shared__ __attribute__((aligned(16))) float2 s_z1[RO_MAX_ENVS][4];          // Z_d^1 of each entry's current state
    __shared__ float s_qv[NACT][RO_MAX_ENVS];                                      // Q_k(s, .) of each live entry
    __shared__ uint16_t s_list[MAX_VF][RO_MAX_ENVS];                               // entry index, per VF k >= 1
    __shared__ int s_cnt[2][MAX_VF];                                               // list lengths, by step parity
    __shared__ float s_clf[MAX_VF * CLF_STRIDE];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int epw = A.epw, N = A.n;
    const int il = wave * epw + lane;                          // this lane's entry within the workgroup (lanes < epw)
    const int i = blockIdx.x * RO_WAVES * epw + il;
    const bool mine = lane < epw && i < N;
    const unsigned known = A.enabled | A.gest;

    // ---- entry: the start state into registers; an entry whose option is not known is not run
    float sx = 0.5f, sy = 0.5f, svx = 0.0f, svy = 0.0f;
    int k = 0;
    if (mine) {
        k = A.option[i];
        if (k >= 1 && k < A.n_vf && ((known >> k) & 1u)) { sx = A.x[i]; sy = A.y[i]; svx = A.vx[i]; svy = A.vy[i]; }
        else k = 0;
    }
    const bool run = k != 0;
    if (!__syncthreads_or(run)) {                              // (workgroup-uniform) nothing to run here
        if (mine) A.out.outcome[i] = 0;
        if constexpr (REC) record_len(kernel_args<TrialRecArgs>()->rec, i, mine, 0);
        return;
    }
    for (int q = tid; q < A.ms.n_edges * 8; q += RO_THREADS) s_edges[q] = A.edges[q];
    if (tid < A.n_vf * CLF_STRIDE) s_clf[tid] = A.clf[tid];
    if (tid < 2 * MAX_VF) (&s_cnt[0][0])[tid] = 0;
    __syncthreads();
    // the entry pass's lists: Q_k(s0, .)
    if (run) store_z1(s_z1[il], sx, sy, svx, svy);
    bool alive = run;
    int par = 0;
#pragma unroll
    for (int kk = 1; kk < MAX_VF; ++kk) list_append(&s_cnt[par][kk], s_list[kk], alive && k == kk, (uint16_t)il, lane);

    float qc[NACT] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float v0 = 0.0f, ret = 0.0f, dret = 0.0f, gk = 1.0f;
    int steps = 0, outcome = 0;
    float *sw = s_wave[wave];
    int rr = -1;                                               // REC: this entry's column in the record, -1: outside its window
    if constexpr (REC) {
        const scg_record R = kernel_args<TrialRecArgs>()->rec;
        if (i - R.first >= 0 && i - R.first < R.n) rr = i - R.first;
    }
    for (;;) {
        __syncthreads();
        // ------------------------------------------------------------ E
        int cnt[MAX_VF], units = 0;
#pragma unroll
        for (int kk = 0; kk < MAX_VF; ++kk) { cnt[kk] = kk >= 1 && kk < A.n_vf ? s_cnt[par][kk] : 0; units += (cnt[kk] + 7) >> 3; }
        if (units == 0) break;                                 // (workgroup-uniform) every trial of the workgroup has ended
        {
            const int n16 = lane & 15, g = lane >> 4, bi = lane & 7, cp = lane >> 3;           // lane roles: scg_eval.hpp
            const int bcol = 8 * (bi >> 2) + (bi & 3);
            const int ocol_item = 4 * (n16 >> 3) + (n16 & 3);
            const bool out_lane = (g == 0) && !(n16 & 4);
            float *cdk = sw, *abq = sw + 36 * 16;
            const float *ab_lane = abq + n16 * AS + 4 * g;
            for (int uu = wave; uu < units; uu += RO_WAVES) {
                int kv = 0, ub = uu;
#pragma unroll
                for (int kk = 0; kk < MAX_VF - 1; ++kk) {
                    const int nu = (cnt[kv] + 7) >> 3;
                    if (ub >= nu) { ub -= nu; ++kv; }
                }
                const int nk = cnt[kv] - 8 * ub;                   // items of this unit still ahead in the list (>= 1)
                const uint16_t *lst = &s_list[kv][8 * ub];
                build_tables(s_z1[lst[min(bi, nk - 1)]], cp, bcol, cdk, abq);
                wave_lds_sync();
                float B[9], q[NACT];
                load_b(cdk, n16, g, B);
                contract_mem<EO_TG>(A.W + (size_t)kv * NACT * NF, B, q, n16, g, ab_lane);
                if (out_lane && ocol_item < nk) {
                    const int ent = lst[ocol_item];
#pragma unroll
                    for (int aa = 0; aa < NACT; ++aa) s_qv[aa][ent] = q[aa];
                }
                wave_lds_sync();                                   // the tables are rewritten by the next unit
            }
        }
        __syncthreads();
        if (tid < MAX_VF) s_cnt[par][tid] = 0;                   // next used two passes on, behind the next pass's barrier
        par ^= 1;
        // ------------------------------------------------------------ G
        if (alive) {
#pragma unroll
            for (int aa = 0; aa < NACT; ++aa) qc[aa] = s_qv[aa][il];
            if (steps == 0) {                                    // the entry pass: SPEC §5's max order
                v0 = qc[0];
#pragma unroll
                for (int aa = 1; aa < NACT; ++aa) v0 = fmaxf(v0, qc[aa]);
            }
        }
        // ------------------------------------------------------------ P: step `steps` at t0 + steps
        const uint64_t t = A.t0 + (uint64_t)steps;
        const uint64_t gid = (uint64_t)(A.env_base + i);
        uint32_t u[4] = {0u, 0u, 0u, 0u};
        int a = NACT - 1;
        if (alive) { env_draw(gid, t, A.seed, u); a = act_spec(u, qc, A.epsilon); }
        float px = sx, py = sy, pvx = svx, pvy = svy;
        bool goal = false;
        const float rew = wave_physics(s_edges, A.cellmask, A.ms, sw, alive, px, py, pvx, pvy, a, goal);
        bool keep = false;
        if (alive) {
            const int dn = episode_end(goal, steps + 1, A.max_ep);
            unsigned inA, inB;
            member_masks(s_clf, A.n_vf, known, px, py, px, py, inA, inB);
            bool succ;
            keep = option_keep(A.parents, k, inA, goal, dn, steps, A.max_opt, succ);
            const float r_o = rew + (succ ? A.r_succ : 0.0f);
            ret = __fadd_rn(ret, r_o);
            dret = __fadd_rn(dret, __fmul_rn(gk, r_o));
            gk = __fmul_rn(gk, A.gamma);
            sx = px; sy = py; svx = pvx; svy = pvy;
            steps += 1;
            if (keep) store_z1(s_z1[il], px, py, pvx, pvy);
            else {                                             // first match wins: succ, done, fail (s' left I_k), time-out
                outcome = succ ? (int)SCG_TRIAL_SUCCESS : dn ? (int)SCG_TRIAL_EPISODE_END
                        : !((inA >> k) & 1u) ? (int)SCG_TRIAL_LEFT_INITIATION : (int)SCG_TRIAL_TIMEOUT;
                alive = false;
            }
            if constexpr (REC) {                                 // SPEC §10's row steps - 1 of this entry
                const scg_record R = kernel_args<TrialRecArgs>()->rec;        // by value: see record_len
                if (rr >= 0 && steps <= R.rows) {
                    const size_t at = (size_t)(steps - 1) * R.n + rr;
                    if (R.x) R.x[at] = px;
                    if (R.y) R.y[at] = py;
                    if (R.vx) R.vx[at] = pvx;
                    if (R.vy) R.vy[at] = pvy;
                    if (R.reward) R.reward[at] = rew;
                    if (R.action) R.action[at] = (uint8_t)a;
                    if (R.done) R.done[at] = (uint8_t)dn;
                    if (R.vf) R.vf[at] = (uint8_t)k;
                    if (R.term) R.term[at] = (uint8_t)(keep ? 0 : outcome);
                    if (R.option_id) R.option_id[at] = (int8_t)k;
                }
            }
        }
#pragma unroll
        for (int kk = 1; kk < MAX_VF; ++kk) list_append(&s_cnt[par][kk], s_list[kk], keep && k == kk, (uint16_t)il, lane);
    }

    // ---- exit: each output once. The pointers are fetched again (kernel_args), as in rollout_kernel, so that the loop does not
    // hold them in scalar registers
    if constexpr (REC) {
        const scg_record R = kernel_args<TrialRecArgs>()->rec;
        record_len(R, i, mine, min(steps, R.rows));                                  // (not run: 0)
    }
    if (!mine) return;
    const scg_trial_out &O = kernel_args<TrialArgs>()->out;
    O.outcome[i] = (uint8_t)outcome;
    if (!run) return;
    if (O.steps) O.steps[i] = steps;
    if (O.ret) O.ret[i] = ret;
    if (O.disc_ret) O.disc_ret[i] = dret;
    if (O.v0) O.v0[i] = v0;
    if (O.end_x) O.end_x[i] = sx;
    if (O.end_y) O.end_y[i] = sy;
    if (O.end_vx) O.end_vx[i] = svx;
    if (O.end_vy) O.end_vy[i] = svy;
}

// the launch of trial_kernel<true, TrialRecArgs>, defined in scg_rollout_variants.hip
__attribute__((visibility("hidden"))) hipError_t launch_trial_record(const TrialRecArgs &A, int grid, hipStream_t s);
