// scg_rollout_kernel.hpp — rollout_kernel: K acting steps (SPEC §8) in ONE launch (included by scg_kernels.hip).
//
// With the weights frozen no env's step reads another env's result, so a workgroup owns a fixed range of RO_WAVES * epw
// consecutive envs (env-id order) for the whole launch and never talks to another workgroup: no grid barrier, no polling,
// no atomics outside LDS. Per step:
//   P  each wave, one lane per env (lanes < epw): act from qcache, Pinball physics on the wave's own (env, edge) pair list
//      (pinball_wave_*), episode bookkeeping, SPEC §4.2 option logic; Z_d^1 of s_next to LDS; the (env, value function)
//      pairs that need Q(s_next, .) — the VF the env runs next, plus the root for an entering env — compacted into one
//      list per value function (ballot / popcount, an LDS counter per list)
//   E  the lists in 8-item units dealt over the workgroup's waves: the E unit of scg_eval.hpp (one table build, then SPEC §3.1's
//      contraction with W_k the A operand: W_0 from LDS, staged once per launch; other VFs straight from memory)
//   G  each lane again: the value gate, the caller-visible ids, qcache, the statistics counters
// State, qcache and counters stay in registers across the steps and are written once at the end. Finished envs (ONE_EPISODE)
// and envs beyond N drop out of the lists; a workgroup with nothing left to step leaves the loop.
#pragma once
#include "scg_wave_phases.hpp"

struct RolloutArgs {
    float *x, *y, *vx, *vy;
    int32_t *option_id, *opt_steps, *ep_steps;
    float *qcache;                 // [5][n]
    uint8_t *action;
    float *reward;
    uint8_t *done;
    const float *W;                // [n_vf][5][1296]
    const float *clf;              // [n_vf][8]
    const float *edges;
    const uint64_t *cellmask;
    const float *starts;
    scg_rollout_stats st;          // device pointers, any may be null
    int32_t n, n_vf, epw, n_steps;
    uint32_t begin, one_episode;
    uint32_t enabled, gest, parents;
    uint64_t t0, seed;
    int64_t env_base;
    float epsilon;
    int32_t max_ep, max_opt;
    uint32_t reoffer_mask;
    MapScalars ms;
    static constexpr bool INT = false;   // SPEC §11's interruption: a compile-time flag of the argument type (kernel symbols unchanged)
    static constexpr bool BEST = false;  // SPEC §14's value-ranked choice: likewise
    static constexpr bool AUDIT = false; // SPEC §15's forced first choice and discounted return: likewise
    static constexpr bool POP = false;   // SPEC §21's population: a weight table, an epsilon and an enabled mask per env range: likewise
    static constexpr bool GATE = false;  // SPEC §25's gate table: the value gate compares under a table of its own: likewise
};
// The fifteen instantiations, the narrowest entry point that launches each (rollout_launch in scg_kernels.hip has the whole mapping), and
// what each adds to <false, RolloutArgs>. INT, BEST, AUDIT and POP are compile-time flags of the argument type. Every argument type has
// RolloutArgs at offset 0, so the exit's re-read holds for all.
//   REC    Args                               launched by                    adds
//   false  RolloutArgs                        scg_rollout                    -
//   false  RolloutIntArgs                     scg_rollout_interrupt          SPEC §11's interruption, counted into `interrupts` (no rec, no BEGIN_AT)
//   true   RolloutVar<false, false, false>    scg_rollout_record             SPEC §10's rows of the envs in the record's window, and BEGIN_AT
//   true   RolloutVar<true,  false, false>    scg_rollout_interrupt          both of the above
//   true   RolloutVar<false, true,  false>    scg_rollout_select, BEST       SPEC §14's value-ranked choice: an offered env is evaluated under
//   true   RolloutVar<true,  true,  false>    ... BEST | INTERRUPT           every candidate's value function and the root's, the Q of VF k in slot k
//                                                                            of s_qv (root: 0); phase G enters the candidate whose value is highest
//   true   RolloutVar<I,     B,     true>     scg_rollout_audit, by `rules`  SPEC §15: the begin pseudo-step's choice may be forced per env, and the
//          (all four I, B)                                                   discounted task return is kept in two more registers across the steps
//                                             scg_rollout_branch             SPEC §19: the same four kernels; the first real step's action may be
//                                                                            given per env (first_action, read on that step only)
//   true   RolloutPop<I, B>                   scg_rollout_population         SPEC §21: the AUDIT kernels over C env ranges of n_per envs, each with
//          (all four I, B; AUDIT)             (pop given)                    its own W, epsilon and enabled mask; a workgroup serves one range, and
//                                                                            the draws are keyed by the env's index within its range
//                                             scg_rollout_population_clf     SPEC §24.1: the same four kernels; with pop_clf a classifier table per
//                                             (pop given)                    range too, staged once per launch in place of `clf`
//   true   RolloutPopGateArgs                 scg_rollout_population_gate    SPEC §25.1: RolloutPop<false, false> whose value gate compares under a
//          (the fifteenth)                    (pop and pop_gate given)       gate table per range, two sides per option, both straight from memory
// Every REC instantiation shares ONE argument layout, RolloutVarArgs (the population's members lie behind it); the
// non-recording interrupting kernel keeps its own, because `interrupts` at another offset changes its code.
struct RolloutIntArgs : RolloutArgs {
    static constexpr bool INT = true;
    int32_t *interrupts;           // [n_vf][N] in/out, may be null
};
struct RolloutVarArgs : RolloutArgs {
    scg_record rec;                // device pointers; n = 0: nothing recorded
    uint32_t begin_at;             // BEGIN's reset replaced by the state given
    int32_t *interrupts;           // [n_vf][N] in/out, may be null (read with INT only)
    int32_t *overrides;            // [n_vf][N] in/out, may be null (read with BEST only)
    scg_audit au;                  // device pointers, any may be null (read with AUDIT only)
    float gamma;
    const uint8_t *first_action;   // [n], may be null (read with AUDIT only): SPEC §19's forced action of the first real step
};
template <bool I, bool B, bool AU>
struct RolloutVar : RolloutVarArgs {
    static constexpr bool INT = I, BEST = B, AUDIT = AU;
};

// SPEC §21: policy c = workgroup / wgs_per_pol acts in the envs c * n_per .. (c + 1) * n_per - 1
struct RolloutPopArgs : RolloutVarArgs {
    int32_t n_pol, n_per;          // n_pol * n_per = n
    int32_t wgs_per_pol;           // ceil(n_per / (RO_WAVES * epw)): a workgroup never straddles two policies
    const float *pol_eps;          // [n_pol], null: epsilon for every policy
    const uint32_t *pol_enabled;   // [n_pol], null: enabled for every policy
    const float *pol_clf;          // [n_pol][n_vf][8], null: clf for every policy (SPEC §24.1; the LAST member: every offset above holds)
};                                 // (W: [n_pol][n_vf][5][1296])
template <bool I, bool B>
struct RolloutPop : RolloutPopArgs {
    static constexpr bool INT = I, BEST = B, AUDIT = true, POP = true;
};
// SPEC §25.1: the gate of option k >= 1 reads max_a Q(s_next, a) under pol_gate[c][k][0] (the option side) against the same under
// pol_gate[c][k][1] (the root side); everything else reads W[c] as before
struct RolloutPopGateArgs : RolloutPopArgs {
    static constexpr bool INT = false, BEST = false, AUDIT = true, POP = true, GATE = true;
    const float *pol_gate;         // [n_pol][n_vf][2][5][1296], never null here (the LAST member: every offset above holds)
};

// per-VF counters of one launch, six 16-bit fields in three words (a launch takes at most 1 + SCG_ROLLOUT_MAX_STEPS steps)
struct Ctr16 {
    uint32_t w[3];
    __device__ __forceinline__ void add(int k, bool on) {
        const uint32_t inc = on ? (1u << (16 * (k & 1))) : 0u;
#pragma unroll
        for (int j = 0; j < 3; ++j) w[j] += (k >> 1) == j ? inc : 0u;
    }
    __device__ __forceinline__ int get(int k) const {
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) v = (k >> 1) == j ? w[j] : v;
        return (int)((v >> (16 * (k & 1))) & 0xffffu);
    }
};
static_assert(SCG_ROLLOUT_MAX_STEPS + 1 < 65536, "16-bit launch counters");

// (the instantiations: the table at the argument types)
template <bool REC, typename Args>
__global__ __launch_bounds__(RO_THREADS) void rollout_kernel(const Args A) {
    constexpr bool INT = Args::INT, BEST = Args::BEST, AUDIT = Args::AUDIT, POP = Args::POP, GATE = Args::GATE;
    static_assert(!GATE || (POP && AUDIT && REC && !INT && !BEST), "the gate table: one instantiation (SPEC §25.1)");
    constexpr int QV_SLOTS = BEST ? MAX_VF : GATE ? 4 : 2;    // BEST: one slot per value function; GATE: [2] / [3] the gate's two sides
    constexpr int QV_ROOT = BEST ? 0 : 1;                     // the slot of the root's Q beside the running VF's
    __shared__ __attribute__((aligned(16))) float s_w0[W_FLOATS];                 // W_0 in A-operand order (stage_w_cold's layout)
    __shared__ __attribute__((aligned(16))) float s_edges[MAX_EDGES * 8];
    __shared__ __attribute__((aligned(16))) float s_wave[RO_WAVES][RO_WAVE_FLOATS];
    __shared__ __attribute__((aligned(16))) float2 s_z1[RO_MAX_ENVS][4];          // Z_d^1 of each env's s_next
    __shared__ float s_qv[QV_SLOTS][NACT][RO_MAX_ENVS];                            // [0]: the VF the env runs next; [1]: the root (entering). BEST: [k]: VF k
    __shared__ uint16_t s_list[MAX_VF][RO_MAX_ENVS];                               // env index | slot << 8
    __shared__ int s_cnt[2][MAX_VF];                                               // list lengths, by step parity
    __shared__ float s_clf[MAX_VF * CLF_STRIDE];
    __shared__ uint16_t s_glist[GATE ? MAX_VF : 1][GATE ? RO_MAX_ENVS : 1];        // GATE: the entering envs by candidate (both sides share a list)
    __shared__ int s_gcnt[2][GATE ? MAX_VF : 1];                                   // GATE: their lengths, by step parity

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int epw = A.epw, N = A.n;
    const int il = wave * epw + lane;                          // this lane's env within the workgroup (lanes < epw)
    // POP (SPEC §21): the workgroup's policy, its weights, epsilon and mask (workgroup-uniform); el: the env's index within the
    // policy's range, which keys its draws; e stays the index of everything in memory
    int pol = 0, el = 0;
    const float *Wp = A.W;
    float epsilon = A.epsilon;
    unsigned enabled = A.enabled;
    if constexpr (POP) {
        pol = (int)(blockIdx.x / (unsigned)A.wgs_per_pol);
        el = ((int)blockIdx.x - pol * A.wgs_per_pol) * RO_WAVES * epw + il;
        Wp = A.W + (size_t)pol * A.n_vf * NACT * NF;
        if (A.pol_eps) epsilon = A.pol_eps[pol];
        if (A.pol_enabled) enabled = A.pol_enabled[pol];
    }
    int n_own = N;                                             // the envs of this workgroup's range
    if constexpr (POP) n_own = A.n_per;
    const int e = POP ? pol * n_own + el : blockIdx.x * RO_WAVES * epw + il;
    const bool mine = lane < epw && (POP ? el : e) < n_own;

    // ---- entry: the env's state into registers
    float sx = 0.5f, sy = 0.5f, svx = 0.0f, svy = 0.0f, qc[NACT] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    int oid = 0, osteps = 0, eps = 0, last_a = 0, last_dn = 0;
    float last_r = 0.0f, ep_ret = 0.0f;
    double ret_sum = 0.0;
    int episodes = 0, goals = 0, len_sum = 0;
    bool finished = false;
    Ctr16 c_vf = {{0u, 0u, 0u}}, c_en = {{0u, 0u, 0u}}, c_de = {{0u, 0u, 0u}}, c_su = {{0u, 0u, 0u}};
    Ctr16 c_in = {{0u, 0u, 0u}};                               // INT: interrupted steps per option
    Ctr16 c_ov = {{0u, 0u, 0u}};                               // BEST: entries of an option that is not min C
    float dsc = 0.0f, dg = 1.0f, dfin = 0.0f;                  // AUDIT: §15's d and g of the running episode; d of the last ended one
    bool have_fin = false;
    if constexpr (AUDIT) {
        if (mine && !A.begin && A.au.disc_ret) { dsc = A.au.disc_ret[e]; dg = A.au.disc_g[e]; }
    }
    if (mine) {
        sx = A.x[e]; sy = A.y[e]; svx = A.vx[e]; svy = A.vy[e];
#pragma unroll
        for (int a = 0; a < NACT; ++a) qc[a] = A.qcache[(size_t)a * N + e];
        oid = A.option_id[e]; osteps = A.opt_steps[e]; eps = A.ep_steps[e];
        if (A.st.finished && !A.begin) finished = A.st.finished[e] != 0;
        if (A.st.ep_return && !A.begin) ep_ret = A.st.ep_return[e];
        if (A.st.ret_sum) ret_sum = A.st.ret_sum[e];
        if (A.st.episodes) episodes = A.st.episodes[e];
        if (A.st.goals) goals = A.st.goals[e];
        if (A.st.len_sum) len_sum = A.st.len_sum[e];
    }
    const bool skip = !mine || (A.one_episode && finished);   // not stepped at all in this launch: nothing of it is written
    if (!__syncthreads_or(!skip)) {                           // (workgroup-uniform) every env of the workgroup is finished
        if constexpr (REC) record_len(kernel_args<RolloutVarArgs>()->rec, e, mine, 0);
        return;
    }
    bool alive = !skip;
    int nrow = 0;                                             // REC: rows recorded
    int rr = -1;                                              // REC: this env's column in the record, -1: outside its window
    if constexpr (REC) {
        const scg_record R = kernel_args<RolloutVarArgs>()->rec;
        if (e - R.first >= 0 && e - R.first < R.n) rr = e - R.first;
    }

    // ---- once per launch: W_0, the edge table and the classifiers to LDS
    for (int i = tid; i < W_FLOATS; i += RO_THREADS) {
        const int z = i - W_TAIL;
        int src;
        const bool in = i < W_TAIL ? w_a_src(i >> 9, 4 * ((i >> 8) & 1) + (i & 3), (i >> 2) & 63, src) : w_a_src(z >> 6, 8, z & 63, src);
        s_w0[i] = in ? Wp[src] : 0.0f;
    }
    for (int i = tid; i < A.ms.n_edges * 8; i += RO_THREADS) s_edges[i] = A.edges[i];
    const float *clfp = A.clf;                                 // POP (SPEC §24.1): the workgroup's policy's table (workgroup-uniform)
    if constexpr (POP) {
        if (A.pol_clf) clfp = A.pol_clf + (size_t)pol * A.n_vf * CLF_STRIDE;
    }
    if (tid < A.n_vf * CLF_STRIDE) s_clf[tid] = clfp[tid];
    if (tid < 2 * MAX_VF) (&s_cnt[0][0])[tid] = 0;
    if constexpr (GATE) {
        if (tid < 2 * MAX_VF) (&s_gcnt[0][0])[tid] = 0;
    }
    __syncthreads();

    const unsigned known = enabled | A.gest;
    const int total = A.n_steps + (A.begin ? 1 : 0);
    float *sw = s_wave[wave];
    for (int j = 0; j < total; ++j) {
        const bool is_begin = A.begin && j == 0;
        const uint64_t t = A.t0 + (uint64_t)j;
        const int par = j & 1;
        // ------------------------------------------------------------ P
        bool valid = alive;
        const uint64_t gid = (uint64_t)(A.env_base + (POP ? el : e));
        uint32_t u[4] = {0u, 0u, 0u, 0u};
        if (valid) env_draw(gid, t, A.seed, u);
        int a = NACT - 1;
        if (valid && !is_begin) a = act_spec(u, qc, epsilon);
        if constexpr (AUDIT) {                                 // SPEC §19: the launch's first real step takes the caller's action
            if (valid && j == (A.begin ? 1 : 0)) {             // (the draw above is made as ever; fetched here, once: see the exit)
                const uint8_t *const fa = kernel_args<Args>()->first_action;
                if (fa) {
                    const int f = fa[e];
                    if (f < NACT) a = f;
                }
            }
        }
        float px = sx, py = sy, pvx = svx, pvy = svy, rew = 0.0f;
        bool goal = false;
        if (!is_begin) rew = wave_physics(s_edges, A.cellmask, A.ms, sw, valid, px, py, pvx, pvy, a, goal);      // (wave-uniform)
        const int o = (oid >= 1 && oid < A.n_vf) ? oid : 0;
        const int eps1 = eps + 1;
        int dn = 0;
        float nx = px, ny = py, nvx = pvx, nvy = pvy;
        bool keep = false, succ = false;
        int cand = 0, on = 0, stay = 0, term = 0;
        int ic = 0;                                            // INT: §4.2's cand of a keeping env, as if its option had ended
        unsigned cset = 0;                                     // BEST: the candidate set C of an env that is not keeping
        int fk = 0, amin = 0;                                  // AUDIT: the force that applies (+k / -k, 0: none) and min C beside it
        if (valid) {
            dn = is_begin ? 2 : episode_end(goal, eps1, A.max_ep);
            if (dn && !(REC && is_begin && kernel_args<RolloutVarArgs>()->begin_at)) restart_state(u[2], A.starts, A.ms.n_starts, nx, ny, nvx, nvy);
            unsigned inA, inB;
            member_masks(s_clf, A.n_vf, known, px, py, nx, ny, inA, inB);
            if (!is_begin && o >= 1) keep = option_keep(A.parents, o, inA, goal, dn, osteps, A.max_opt, succ);
            if (REC && !is_begin && o >= 1 && !keep)          // SPEC §9's outcome code, first match wins
                term = succ ? (int)SCG_TRIAL_SUCCESS : dn ? (int)SCG_TRIAL_EPISODE_END
                     : !((inA >> o) & 1u) ? (int)SCG_TRIAL_LEFT_INITIATION : (int)SCG_TRIAL_TIMEOUT;
            cand = keep ? o : select_option(A.parents, inB, enabled);
            if constexpr (INT) ic = keep ? select_option(A.parents, inB, enabled) : 0;
            if constexpr (BEST) {                              // SPEC §14: stay out of ANY member of C; cand = that member
                cset = keep ? 0u : candidate_mask(A.parents, inB, enabled);
                const int o_in = is_begin ? 0 : oid;
                const bool out_of = o_in < 0 && o_in > -MAX_VF && ((cset >> (unsigned)(-o_in & 7)) & 1u);
                stay = (!keep && out_of && dn == 0 && (((uint32_t)t + (uint32_t)gid) & A.reoffer_mask) != 0u) ? -o_in : 0;
                if (stay) cand = stay;
            } else {
                stay = reoffer_stay(keep, cand, dn, is_begin ? 0 : oid, t, gid, A.reoffer_mask);
            }
            if constexpr (AUDIT) {                             // SPEC §15: the begin choice forced to a member of C (begin: stay = 0)
                if (is_begin && A.au.force) {
                    const int f = A.au.force[e], k = f < 0 ? -f : f;
                    const unsigned C = BEST ? cset : candidate_mask(A.parents, inB, enabled);
                    if (k >= 1 && k < A.n_vf && ((C >> k) & 1u)) {
                        fk = f; amin = cand; cand = k;
                        if constexpr (BEST) cset = 1u << k;    // phase E's lists: Q_k and Q_0 of this env, no other
                    }
                }
            }
            on = stay ? 0 : cand;
            store_z1(s_z1[il], nx, ny, nvx, nvy);
        }
        const bool entering = valid && !keep && on >= 1;
        // compaction: slot 0 -> the list of VF `on`, slot 1 (entering; INT: keeping too) -> the root's list. An env is entering
        // or keeping, never both, and either way runs on >= 1 next: the root's list still holds at most one item per env
        if constexpr (BEST) {
            // slot = VF index. An offered env goes to the list of every k in C and to the root's; a keeping env to its option's
            // (INT: and the root's); any other to the root's. Every list still holds at most one item per env
            const unsigned want = !valid ? 0u : entering ? (cset | 1u) : keep ? ((1u << o) | (INT ? 1u : 0u)) : 1u;
#pragma unroll
            for (int k = 0; k < MAX_VF; ++k)
                list_append(&s_cnt[par][k], s_list[k], (want >> k) & 1u, (uint16_t)(il | (k << 8)), lane);
        } else
#pragma unroll
        for (int k = 0; k < MAX_VF; ++k) {
            const bool w0 = valid && on == k, w1 = (entering || (INT && keep)) && k == 0;
            const uint64_t b0 = __ballot(w0), b1 = __ballot(w1);
            const int n0 = __popcll(b0), n1 = __popcll(b1);
            if (n0 + n1 == 0) continue;                         // (wave-uniform)
            int base = 0;
            if (lane == 0) base = atomicAdd(&s_cnt[par][k], n0 + n1);       // ONE atomic for both slots (the trial's single append: list_append)
            base = __shfl(base, 0, 64);
            const uint64_t below = (1ull << lane) - 1ull;
            if (w0) s_list[k][base + __popcll(b0 & below)] = (uint16_t)il;
            if (w1) s_list[k][base + n0 + __popcll(b1 & below)] = (uint16_t)(il | 0x100);
        }
        if constexpr (GATE) {                                  // SPEC §25.1: an entering env also goes to the gate list of its cand (= on)
#pragma unroll
            for (int k = 1; k < MAX_VF; ++k) list_append(&s_gcnt[par][k], s_glist[k], entering && on == k, (uint16_t)il, lane);
        }
        __syncthreads();
        // ------------------------------------------------------------ E
        int cnt[MAX_VF], units = 0;
#pragma unroll
        for (int k = 0; k < MAX_VF; ++k) { cnt[k] = k < A.n_vf ? s_cnt[par][k] : 0; units += (cnt[k] + 7) >> 3; }
        [[maybe_unused]] int gcnt[GATE ? MAX_VF : 1], gunits = 0;              // GATE: the gate lists and their units (every one also has an ordinary unit)
        if constexpr (GATE) {
            gcnt[0] = 0;
#pragma unroll
            for (int k = 1; k < MAX_VF; ++k) { gcnt[k] = k < A.n_vf ? s_gcnt[par][k] : 0; gunits += (gcnt[k] + 7) >> 3; }
        }
        if (units + gunits == 0) break;                        // (workgroup-uniform) nothing left to step
        {
            const int n16 = lane & 15, g = lane >> 4, bi = lane & 7, cp = lane >> 3;           // lane roles: scg_eval.hpp
            const int bcol = 8 * (bi >> 2) + (bi & 3);
            const int ocol_item = 4 * (n16 >> 3) + (n16 & 3);
            const bool out_lane = (g == 0) && !(n16 & 4);
            float *cdk = sw, *abq = sw + 36 * 16;
            const float *ab_lane = abq + n16 * AS + 4 * g;
            const f4v *w4 = reinterpret_cast<const f4v *>(s_w0) + lane;
            const float *w8 = s_w0 + W_TAIL + lane;
            for (int uu = wave; uu < units; uu += RO_WAVES) {
                int k = 0, ub = uu;
#pragma unroll
                for (int kk = 0; kk < MAX_VF - 1; ++kk) {
                    const int nu = (cnt[k] + 7) >> 3;
                    if (ub >= nu) { ub -= nu; ++k; }
                }
                const int nk = cnt[k] - 8 * ub;                    // items of this unit still ahead in the list (>= 1)
                const uint16_t *lst = &s_list[k][8 * ub];
                build_tables(s_z1[lst[min(bi, nk - 1)] & 0xff], cp, bcol, cdk, abq);
                wave_lds_sync();
                float B[9], q[NACT];
                load_b(cdk, n16, g, B);
                if (k == 0) contract_lds<E_TG>(0, B, q, g, w4, w8, ab_lane);      // W_0 from LDS
                else contract_mem<EO_TG>(Wp + (size_t)k * NACT * NF, B, q, n16, g, ab_lane);      // W_k straight from memory (L2-resident: 26 KB per VF)
                if (out_lane && ocol_item < nk) {
                    const int ent = lst[ocol_item];
#pragma unroll
                    for (int aa = 0; aa < NACT; ++aa) s_qv[ent >> 8][aa][ent & 0xff] = q[aa];
                }
                wave_lds_sync();                                   // the tables are rewritten by the next unit
            }
            if constexpr (GATE) {
                // SPEC §25.1: the gate lists behind the ordinary units, dealt on from the wave those ended at. ONE table build per
                // unit, then both sides of option k's comparison from memory, into slots 2 (option side) and 3 (root side)
                const float *gp = kernel_args<Args>()->pol_gate + (size_t)pol * A.n_vf * 2 * NACT * NF;
                for (int uu = (wave + RO_WAVES - units % RO_WAVES) % RO_WAVES; uu < gunits; uu += RO_WAVES) {
                    int k = 1, ub = uu, ck = gcnt[1];              // (gcnt by constant indices only: it stays in registers)
                    bool on_k = false;
#pragma unroll
                    for (int kk = 1; kk < MAX_VF - 1; ++kk) {
                        const int nu = (gcnt[kk] + 7) >> 3;
                        on_k = on_k || ub < nu;
                        if (!on_k) { ub -= nu; k = kk + 1; ck = gcnt[kk + 1]; }
                    }
                    const int nk = ck - 8 * ub;                    // items of this unit still ahead in the list (>= 1)
                    const uint16_t *lst = &s_glist[k][8 * ub];
                    build_tables(s_z1[lst[min(bi, nk - 1)] & 0xff], cp, bcol, cdk, abq);
                    wave_lds_sync();
                    float B[9], q[NACT];
                    load_b(cdk, n16, g, B);
#pragma unroll 1
                    for (int side = 0; side < 2; ++side) {
                        contract_mem<EO_TG>(gp + ((size_t)k * 2 + side) * NACT * NF, B, q, n16, g, ab_lane);
                        if (out_lane && ocol_item < nk) {
                            const int ent = lst[ocol_item];
#pragma unroll
                            for (int aa = 0; aa < NACT; ++aa) s_qv[2 + side][aa][ent] = q[aa];
                        }
                    }
                    wave_lds_sync();
                }
            }
        }
        __syncthreads();
        if (tid < MAX_VF) s_cnt[par][tid] = 0;                   // next used at step j + 2, behind step j + 1's barrier
        if constexpr (GATE) {
            if (tid < MAX_VF) s_gcnt[par][tid] = 0;
        }
        // ------------------------------------------------------------ G
        if (valid) {
            float qa[NACT];
            int minc = cand;                                   // BEST: min C of an offered env
            if constexpr (BEST) {
                if (entering) {                                // SPEC §14: c* = the candidate of the highest value, ties to the lowest k
                    float vbest = 0.0f;
                    int cs = 0;
#pragma unroll
                    for (int k = 1; k < MAX_VF; ++k) {
                        if ((cset >> k) & 1u) {
                            float v = s_qv[k][0][il];
#pragma unroll
                            for (int aa = 1; aa < NACT; ++aa) v = fmaxf(v, s_qv[k][aa][il]);      // gate_holds' order
                            if (v == v && (cs == 0 || v > vbest)) { vbest = v; cs = k; }          // a NaN never wins
                        }
                    }
                    cand = cs ? cs : minc;                     // every value a NaN: min C (the gate then declines it)
                }
                const int slot = entering ? cand : on;         // keeping: on = o; staying, no candidate: 0
#pragma unroll
                for (int aa = 0; aa < NACT; ++aa) qa[aa] = s_qv[slot][aa][il];
            } else {
#pragma unroll
                for (int aa = 0; aa < NACT; ++aa) qa[aa] = s_qv[0][aa][il];
            }
            bool declined = false;
            if (entering) {
                float q0[NACT];
#pragma unroll
                for (int aa = 0; aa < NACT; ++aa) q0[aa] = s_qv[QV_ROOT][aa][il];
                [[maybe_unused]] float gk[GATE ? NACT : 1];                    // GATE: Q(s_next, .) under the option side of cand's gate
                if constexpr (GATE) {                          // SPEC §25.1: the comparison alone moves to the gate table's two sides
                    float g0[NACT];
#pragma unroll
                    for (int aa = 0; aa < NACT; ++aa) { gk[aa] = s_qv[2][aa][il]; g0[aa] = s_qv[3][aa][il]; }
                    declined = !gate_holds(gk, g0);
                } else {
                    declined = !gate_holds(qa, q0);
                }
                if constexpr (AUDIT) {
                    if (is_begin) {                            // SPEC §15's begin outputs, from the values the gate reads
                        const scg_audit U = kernel_args<Args>()->au;
                        float v = qa[0];
                        if constexpr (GATE) v = gk[0];
#pragma unroll
                        for (int aa = 1; aa < NACT; ++aa) {
                            if constexpr (GATE) v = fmaxf(v, gk[aa]);
                            else v = fmaxf(v, qa[aa]);
                        }
                        if (U.v_cand) U.v_cand[e] = v;
                    }
                    if (fk) declined = fk < 0;                 // the force replaces the gate's result
                }
                if (declined) {
#pragma unroll
                    for (int aa = 0; aa < NACT; ++aa) qa[aa] = q0[aa];
                }
            }
            bool interrupted = false;                          // SPEC §11: the gate's comparison on every step an option goes on
            if constexpr (INT) {
                if (keep) {
                    float q0[NACT];
#pragma unroll
                    for (int aa = 0; aa < NACT; ++aa) q0[aa] = s_qv[QV_ROOT][aa][il];
                    interrupted = !gate_holds(qa, q0);         // V_o against V_0 at s_next: ties keep the option
                    if (interrupted) {
#pragma unroll
                        for (int aa = 0; aa < NACT; ++aa) qa[aa] = q0[aa];
                    }
                }
            }
#pragma unroll
            for (int aa = 0; aa < NACT; ++aa) qc[aa] = qa[aa];
            sx = nx; sy = ny; svx = nvx; svy = nvy;
            oid = (declined || stay) ? -cand : cand;
            osteps = keep ? osteps + 1 : 0;
            if constexpr (INT) {
                if (interrupted) { oid = -ic; osteps = 0; }    // the root runs, staying out of ic (0: none) until its re-offer
                c_in.add(o, interrupted);
                if (interrupted) term = (int)SCG_ROLLOUT_TERM_INTERRUPTED;
            }
            eps = dn ? 0 : eps1;
            c_en.add(cand, entering && !declined);
            c_de.add(cand, declined);
            if constexpr (AUDIT) {
                if (fk) minc = amin;                           // a forced entry overrides where k != min C
                if (is_begin) {
                    const scg_audit U = kernel_args<Args>()->au;
                    constexpr int QV_VROOT = GATE ? 3 : QV_ROOT;  // GATE: the root side of the gate an entering env was offered
                    float v = s_qv[entering ? QV_VROOT : 0][0][il];
#pragma unroll
                    for (int aa = 1; aa < NACT; ++aa) v = fmaxf(v, s_qv[entering ? QV_VROOT : 0][aa][il]);
                    if (U.v_root) U.v_root[e] = v;
                    if (U.cand) U.cand[e] = (int8_t)(entering ? cand : 0);
                    if (U.applied) U.applied[e] = fk ? 1 : 0;
                }
            }
            if constexpr (BEST) c_ov.add(cand, entering && !declined && cand != minc);
            if (!is_begin) {
                last_a = a; last_r = rew; last_dn = dn;
                c_vf.add(o, true);
                c_su.add(o, o >= 1 && succ);
                if constexpr (AUDIT) {                         // SPEC §15: d += g * reward, g *= gamma, each rounded, no fma
                    dsc = __fadd_rn(dsc, __fmul_rn(dg, rew));
                    dg = __fmul_rn(dg, A.gamma);
                    if (dn) { dfin = dsc; have_fin = true; dsc = 0.0f; dg = 1.0f; }
                }
                const float r = ep_ret + rew;
                if (dn) {
                    episodes += 1; goals += dn == 1 ? 1 : 0; len_sum += eps1;
                    ret_sum = ret_sum + (double)r;
                    ep_ret = 0.0f;
                    finished = true;
                    if (A.one_episode) alive = false;
                } else {
                    ep_ret = r;
                }
            } else {
                ep_ret = 0.0f;
                finished = false;
                if constexpr (AUDIT) { dsc = 0.0f; dg = 1.0f; }
            }
            if constexpr (REC) {                                 // SPEC §10's row j of this env
                if (rr >= 0) {
                    const scg_record R = kernel_args<RolloutVarArgs>()->rec;  // by value: see record_len
                    const size_t at = (size_t)j * R.n + rr;
                    if (R.x) R.x[at] = is_begin ? sx : px;
                    if (R.y) R.y[at] = is_begin ? sy : py;
                    if (R.vx) R.vx[at] = is_begin ? svx : pvx;
                    if (R.vy) R.vy[at] = is_begin ? svy : pvy;
                    if (R.reward) R.reward[at] = rew;
                    if (R.action) R.action[at] = is_begin ? (uint8_t)255 : (uint8_t)a;
                    if (R.done) R.done[at] = (uint8_t)dn;
                    if (R.vf) R.vf[at] = is_begin ? (uint8_t)0 : (uint8_t)o;
                    if (R.term) R.term[at] = (uint8_t)term;
                    if (R.option_id) R.option_id[at] = (int8_t)oid;
                }
                nrow += 1;
            }
        }
    }

    // ---- exit: the stepped envs' results, once. The output pointers are fetched from the kernel arguments again here (kernel_args):
    // otherwise the compiler keeps the 21 pointers it loaded at entry live in scalar registers across the whole step loop
    if constexpr (REC) record_len(kernel_args<RolloutVarArgs>()->rec, e, mine, nrow);     // (skipped: 0)
    if (skip) return;
    const RolloutArgs *K = kernel_args<RolloutArgs>();
    K->x[e] = sx; K->y[e] = sy; K->vx[e] = svx; K->vy[e] = svy;
#pragma unroll
    for (int a = 0; a < NACT; ++a) K->qcache[(size_t)a * N + e] = qc[a];
    K->option_id[e] = oid; K->opt_steps[e] = osteps; K->ep_steps[e] = eps;
    if (K->n_steps > 0) { K->action[e] = (uint8_t)last_a; K->reward[e] = last_r; K->done[e] = (uint8_t)last_dn; }
    const scg_rollout_stats &S = K->st;
    if (S.ep_return) S.ep_return[e] = ep_ret;
    if (S.ret_sum) S.ret_sum[e] = ret_sum;
    if (S.episodes) S.episodes[e] = episodes;
    if (S.goals) S.goals[e] = goals;
    if (S.len_sum) S.len_sum[e] = len_sum;
    if (S.finished) S.finished[e] = finished ? 1 : 0;
    for (int k = 0; k < K->n_vf; ++k) {
        const size_t at = (size_t)k * N + e;
        if (S.vf_steps) S.vf_steps[at] += c_vf.get(k);
        if (S.entries) S.entries[at] += c_en.get(k);
        if (S.declines) S.declines[at] += c_de.get(k);
        if (S.successes) S.successes[at] += c_su.get(k);
    }
    if constexpr (INT) {
        int32_t *const I = kernel_args<Args>()->interrupts;
        if (I)
            for (int k = 0; k < K->n_vf; ++k) I[(size_t)k * N + e] += c_in.get(k);
    }
    if constexpr (AUDIT) {
        const scg_audit U = kernel_args<Args>()->au;
        if (U.disc_ret) { U.disc_ret[e] = dsc; U.disc_g[e] = dg; }
        if (U.disc_final && have_fin) U.disc_final[e] = dfin;
    }
    if constexpr (BEST) {
        int32_t *const O = kernel_args<Args>()->overrides;
        if (O)
            for (int k = 0; k < K->n_vf; ++k) O[(size_t)k * N + e] += c_ov.get(k);
    }
}

// the launch of rollout_kernel<REC, Args>: defined and instantiated in scg_rollout_variants.hip for every Args but RolloutArgs
template <bool REC, typename Args>
__attribute__((visibility("hidden"))) hipError_t launch_rollout(const Args &A, int grid, hipStream_t s);
