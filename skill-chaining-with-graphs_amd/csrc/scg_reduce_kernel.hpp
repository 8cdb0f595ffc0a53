// scg_reduce_kernel.hpp — the reduce launch of a step-batch (SPEC §5): reduce_kernel<8 | 16> and, for acting-only steps, commit_kernel.
// Included by scg_kernels.hip behind scg_order.hpp and scg_collect_kernels.hpp.
#pragma once

// slabs -> G (SPEC §5 two-level block order), n_k, optional apply; the next step's env order rides along
struct ReduceArgs {
    const float *slabs;
    const int32_t *cnts;
    float *G;
    int32_t *n_k;
    float *nk_f;             // packed operand: the counts again, as floats right after G (null = off)
    float *W;
    const float *scale;
    int32_t nblk, n_vf;
    float alpha;
    uint32_t apply;
    int32_t nk_floor;              // SPEC §5 apply: divisor max(n_k, nk_floor)
    // next step's env order (SPEC §5) as extra workgroups (option_id null = off): the fused kernel has counted
    // the new option ids per row of 256 envs into `hist`; `hist_zero` is the other buffer, cleared for the next step
    const int32_t *option_id;
    int32_t *hist, *hist_zero, *perm;
    int32_t n, nrow;
    // commit of the fused kernel's per-position results to the caller's arrays (outrec null = off), one row of
    // 256 envs per wave; with `sort` the same wave then places its row in the next env order
    const float4 *outrec;
    const float4 *qalt;            // the root's Q(s', .) of the envs whose result line carries the declined mark (SPEC §4.2); never null where outrec is set
    int32_t *invperm;              // [n] position of env e in the current order (in: this step's, out: the next's)
    float *x, *y, *vx, *vy, *reward;
    int32_t *option_id_out, *opt_steps, *ep_steps;
    uint8_t *action, *done;
    float *qcache;                 // [5][n], null = the step ran no TD pass (diagnostic): leave it alone
    int32_t sort;
    const int32_t *fail_flag;      // set by a workgroup of the step kernel that gave up: the step is void (no apply, no commit)
    // an announced example trigger (scg_arm_collect; c_rows null = none): the commit rows leave what collect_count_kernel would
    const uint8_t *c_events, *c_prev;
    const int32_t *c_evlen, *c_count;
    int32_t *c_rows;
    uint32_t c_bits;
    int32_t c_L, c_ring_len;
#ifdef SCG_REDUCE_STAMPS
    unsigned long long *stamps;    // diagnostic build: [workgroup][RED_STAMP_SLOTS] (RED_STAMP below)
#endif
};

constexpr int SEG = 16;            // SPEC §5: blocks per first-level segment
constexpr int RED_ROUND = 32;      // segments per round of the kernel (512 blocks)
constexpr int RED_SPW = 2;         // segments per lane group and round
constexpr int RED_GROUPS = RED_ROUND / RED_SPW;                      // lane groups per slab workgroup: one segment each per pass
constexpr int RED_COLS = NACT * NF / 4;                              // float4 columns per value function
// A slab workgroup owns RED_C float4 columns of one value function; a wave's 64 lanes are RED_GPW lane groups of RED_C columns, and
// lane group g of the workgroup sums the segments g and RED_GROUPS + g of a round: four waves of four groups. (Round 18; before it a
// workgroup was sixteen waves on 64 columns, and the root's 256 KB per workgroup went through one CU's load path.) A row workgroup
// is exactly its four waves.
constexpr int RED_C = 16;
constexpr int RED_GPW = 64 / RED_C;                                  // lane groups per wave
constexpr int RED_WAVES = RED_GROUPS / RED_GPW;
constexpr int RED_THREADS = 64 * RED_WAVES;
constexpr int RED_NCOL = (RED_COLS + RED_C - 1) / RED_C;             // grid.x: column chunks (the last one partial)
// diagnostic build: [0] entry, [1] exit (row workgroups: [1..4] = waves 0..3, [5] wave 0's record arrived, [6] wave 0 behind the
// barrier), slab wave 0: [5] sums parked, [6] barrier passed, [7] G summed; slab wave w: [8 + w] its last round's sums parked
constexpr int RED_STAMP_SLOTS = 24;

// the hardware lane counter. Lane-derived indices and addresses of the slab half are re-made from it where they are used: as values
// of the kernel's one `lane`, live from the top to the last store, five of them were kept in scratch at 64 VGPRs, and each reload's
// s_waitcnt vmcnt(0) put a memory round trip of its own in front of a count load (run_pass re-makes its lane ids for the same reason)
__device__ __forceinline__ int lane_now() {
    int ln;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
    return ln;
}

// integer sum over each row of 16 lanes, left in every lane of the row: four DPP adds, no LDS round trip (integers: any order)
__device__ __forceinline__ int row_sum(int v) {
    v += __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true);      // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, true);      // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_mov_dpp(v, 0x141, 0xF, 0xF, true);     // row_half_mirror
    v += __builtin_amdgcn_mov_dpp(v, 0x140, 0xF, 0xF, true);     // row_mirror
    return v;
}

// lane 16 r + j holds a value of row r: the sum over the four rows, left in all four of them. Two lane swaps in the vector pipe:
// v_permlane32_swap exchanges the upper half of its first operand with the lower half of its second, v_permlane16_swap the odd rows
// of the first with the even rows of the second
__device__ __forceinline__ int rows_sum(int v) {
    const auto h = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
    v = (int)(h[0] + h[1]);
    const auto q = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
    return (int)(q[0] + q[1]);
}

// diagnostic build (make rstamps; tools/reduce_chain.py): every workgroup leaves the 100 MHz clock at entry, at exit and at the
// steps in between that RED_STAMP_SLOTS lists. Not in the product: the macros are empty and ReduceArgs has no such field.
#ifdef SCG_REDUCE_STAMPS
#define RED_STAMP(slot) do { \
        if (R.stamps && lane_now() == 0) \
            R.stamps[(size_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.y * gridDim.x + blockIdx.x) * RED_STAMP_SLOTS + (slot))] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
#define RED_STAMP_DRAINED(slot) do { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); RED_STAMP(slot); } while (0)
#else
#define RED_STAMP(slot) do { } while (0)
#define RED_STAMP_DRAINED(slot) do { } while (0)
#endif

// Four waves per row of 256 envs (wave wv owns envs 64 wv .. 64 wv + 63 of the row):
//   commit: gather each env's result line from its position in the current order (one 64-byte read) and write
//           the caller's SoA arrays (state, outputs, qcache) with full-line stores;
//   sort  : place the row in the stable counting-sort order of the next step (7 keys), from the per-row key
//           counts of all rows: offset(key k, row) = (envs with a smaller key) + (key-k envs of earlier rows)
//           (+ key-k envs of the row's earlier waves, exchanged through LDS together with the waves' shares of the
//           count table).
// Every thread of the workgroup must call this (it holds the barrier); waves >= 4 only pass through it.
// The chain of a wave is two dependent memory round trips and one workgroup barrier:
//   1  the env's position (invperm[e]), with the failed-step flag and the wave's quarter of the count table beside it. The table's
//      loop has a run-time trip count and ends on a full wait, so the position has arrived when it is left;
//   2  the result line's four words AND the two words of qalt at the same position, all six issued back to back. qalt is read for
//      every env, not only for a declined one (which would be a third round trip behind the record's mark): the position is in
//      bounds of qalt for every env, and what a line of an env that was not declined holds is dropped by the select below.
//      The fourteen table sums over the wave run while these are in flight, in the vector pipe (DPP row sums and two lane swaps:
//      no LDS round trip);
//   -  the SoA stores, the key ballots, the wave's 21 exchange words to LDS, and a barrier that waits for LDS only: nothing that
//      goes through global memory crosses it (every lane reads and later writes its own invperm[e] and no other), so the stores'
//      acknowledgements are not waited for in front of it;
//   -  behind the barrier the order from the LDS words, perm / invperm stores.
// An announced trigger (c_rows) adds its own loads and their wait in front of the barrier; it is finished inside its branch.
// One wave per row (four envs per lane) took 8.3 us of dependent work after the launch floor; see DESIGN §10.
__device__ __forceinline__ void commit_and_place_row(const ReduceArgs &R, int row, int wv, int lane, int (*s_x)[40]) {
    // a workgroup of this step gave up (uniform): the caller's arrays and the env order keep what the previous step left. The flag is
    // FETCHED here and looked at where the first result would be written: a test up front put one more dependent round trip in front
    // of everything the row does (+1.9 us per step-batch)
    // (read through a per-lane zero offset: as a wave-uniform load the compiler turns it into a scalar at once — global_load, s_waitcnt
    //  vmcnt(0), v_readfirstlane — which is the up-front test again)
    int zoff = 0;
    asm volatile("" : "+v"(zoff));
    const int step_failed = R.fail_flag[zoff];              // (never null: the context's flag word)
    const bool act = wv < 4 && row < R.nrow;
    const int e = row * 256 + wv * 64 + lane;
    const bool ok = act && e < R.n;
    // the position is used only by lanes that are `ok`; the others read the flag word again. (As `ok ? invperm[e] : 0` the load sits in a
    //  branch of its own whose end waits for it, and the count table's loads, which do not need the position, issue behind that wait
    //  instead of beside the load. Unsigned: no sign extension to wait for either.)
    const unsigned pos_old = (unsigned)*(ok ? R.invperm + e : R.fail_flag);
    int tot[NKEY], pre[NKEY];
#pragma unroll
    for (int k = 0; k < NKEY; ++k) { tot[k] = 0; pre[k] = 0; }
    if (act && R.sort) {
        for (int r = wv * 64 + lane; r < R.nrow; r += 256) {       // this wave's quarter of the count table
#pragma unroll
            for (int k = 0; k < NKEY; ++k) {
                const int h = R.hist[r * HSTRIDE + k];
                tot[k] += h;
                if (r < row) pre[k] += h;
            }
        }
    }
    float4 ra = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rb = ra, rq = ra, r3 = ra, qa = ra;
    float qb = 0.0f;
    if (ok) {
        const float4 *r = R.outrec + (size_t)pos_old * OREC;
        const float4 *q = R.qalt + (size_t)pos_old * 2;
        ra = r[0]; rb = r[1]; rq = r[2]; r3 = r[3];
        qa = q[0]; qb = q[1].x;
    }
    int tsum = 0;                                           // lanes 0..NKEY-1: the table's key totals, NKEY..2 NKEY-1: those of the rows before this one
    if (act && R.sort) {                                    // (integer sums: any order) under the record's round trip
        const int j = lane & 15;
#pragma unroll
        for (int k = 0; k < NKEY; ++k) {
            const int t = row_sum(tot[k]), p = row_sum(pre[k]);
            if (j == k) tsum = t;
            if (j == NKEY + k) tsum = p;
        }
        tsum = rows_sum(tsum);
    }
#ifdef SCG_REDUCE_STAMPS
    if (wv == 0 && act) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); RED_STAMP(5); }
#endif
    // (the record's first use hangs on the sums: left to itself the compiler tests the mark inside the branch that loads it, with a
    //  wait in front of the sums. The line's two unused words are held until here as well: a loaded register that nobody reads is
    //  handed out again while the load is in flight, and its next writer — one of the sums — waits for the load. So is the position:
    //  on the path of a lane that is not `ok` its load counts as in flight, and a sum that took its register waited for everything)
    unsigned mark = __float_as_uint(r3.y);
    asm volatile("" : "+v"(mark), "+v"(tsum) : "v"(r3.z), "v"(r3.w), "v"(pos_old));
    float q4 = r3.x;
    if (ok && mark == OREC_DECLINED) {                      // SPEC §4.2: the option promised less than the root — the env stays with the root
        rq = qa; q4 = qb;
        rb.y = __uint_as_float(__float_as_uint(rb.y) | 0x01000000u);      // declined: bit 24 of the record's bits
    }
    int key = -1;
    uint64_t km[NKEY];
    if (act) {
        const unsigned bits = __float_as_uint(rb.y);
        if (ok && !step_failed) {
            const int on = (int)((bits >> 16) & 255u);
            const bool declined = (bits >> 24) & 1u;            // set above from the result line's mark (SPEC §4.2): declined in this step
            // the caller sees -k: inside option k's initiation set, staying out of it (bits 28..30: it has been since an earlier step)
            const int oid = declined ? -on : (on ? on : -(int)((bits >> 28) & 7u));
            key = sort_key(oid, R.n_vf);
            R.x[e] = ra.x; R.y[e] = ra.y; R.vx[e] = ra.z; R.vy[e] = ra.w;
            R.reward[e] = rb.x; R.action[e] = (uint8_t)(bits & 255u); R.done[e] = (uint8_t)((bits >> 8) & 255u);
            R.option_id_out[e] = oid; R.opt_steps[e] = __float_as_int(rb.z); R.ep_steps[e] = __float_as_int(rb.w);
            if (R.qcache) {
                const size_t n = (size_t)R.n;
                R.qcache[e] = rq.x; R.qcache[n + e] = rq.y; R.qcache[2 * n + e] = rq.z;
                R.qcache[3 * n + e] = rq.w; R.qcache[4 * n + e] = q4;
            }
        }
        if (R.sort) {
#pragma unroll
            for (int k = 0; k < NKEY; ++k) km[k] = __ballot(key == k);
            if (lane < 3 * NKEY) {                          // [0..NKEY) table totals, [NKEY..2 NKEY) rows before this one, [2 NKEY..3 NKEY) this wave's keys
                int v = tsum;
#pragma unroll
                for (int k = 0; k < NKEY; ++k)
                    if (lane == 2 * NKEY + k) v = __popcll(km[k]);
                s_x[wv][lane] = v;
            }
        }
    }
    if (R.c_rows && act) {                                  // the announced trigger's examples of this wave's envs (SPEC §7)
        bool in;
        const int v = rows_sum(row_sum(collect_v(e, R.n, R.c_events, R.c_prev, R.c_bits, R.c_evlen, R.c_ring_len, R.c_L, in)));
        if (lane == 0) s_x[wv][3 * NKEY] = v;
    }
    if (!R.sort && !R.c_rows) return;                       // workgroup-uniform
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");      // LDS words only (above): no wait for the SoA stores' acknowledgements
#ifdef SCG_REDUCE_STAMPS
    if (wv == 0 && act) RED_STAMP(6);
#endif
    if (R.c_rows && wv == 0 && lane == 0 && row < R.nrow) {
        R.c_rows[row] = s_x[0][3 * NKEY] + s_x[1][3 * NKEY] + s_x[2][3 * NKEY] + s_x[3][3 * NKEY];
        if (row == 0) R.c_rows[R.nrow] = *R.c_count;        // the buffer's fill level
    }
    if (!R.sort || !act) return;
    int off[NKEY];
#pragma unroll
    for (int k = 0; k < NKEY; ++k) {
        tot[k] = s_x[0][k] + s_x[1][k] + s_x[2][k] + s_x[3][k];
        off[k] = s_x[0][NKEY + k] + s_x[1][NKEY + k] + s_x[2][NKEY + k] + s_x[3][NKEY + k];
#pragma unroll
        for (int w = 0; w < 3; ++w) off[k] += w < wv ? s_x[w][2 * NKEY + k] : 0;      // rank of this wave's first key-k env within its run
    }
    OrderLayout L;
    order_layout(tot, R.n, L);
    int rk = -1, st = 0;
#pragma unroll
    for (int k = 0; k < NKEY; ++k)
        if (key == k) { rk = off[k] + __popcll(km[k] & ((1ull << lane) - 1ull)); st = L.start[k]; }
    if (rk >= 0 && !step_failed) {
        const int pos = key == 0 ? order_pos0(L, rk) : order_posk(L, st, rk);
        R.perm[pos] = e; R.invperm[e] = pos;
    }
    if (wv == 0 && lane < HSTRIDE) R.hist_zero[row * HSTRIDE + lane] = 0;
}

// grid (column chunks, [rows of the env order +] n_vf). A workgroup owns RED_C float4 columns of one value function; each of
// its RED_GROUPS lane groups sums one segment's slabs per pass, T_s = ((P_16s + P_16s+1) + ...) over the non-empty blocks with BATCH
// loads in flight, and parks T_s in LDS; wave 0 adds the segments in order, G = ((T_0 + T_1) + ...)
// — SPEC §5's two levels in one launch.
// BATCH = slab loads in flight per wave: 16 (one memory round trip per segment — for small launches, see launch_reduce) or 8
// (64 VGPRs, eight waves per SIMD: the bench size's workgroups are resident together). The sum runs in block order either way:
// same bits.
// The lane groups of a wave hold slabs in different blocks: a slab load is issued where any group of the wave has one
// (wave-uniform test) and executed by the lanes whose own group has (the others keep +0), and every
// lane adds all of the batch. The +0 terms leave the bits alone: T starts at +0 and x + y is -0 only where both are, so T is never
// -0 and T + (+0) == T for every value T can hold, Inf and NaN included (the second level's argument, below).
// A slab workgroup's chain is: the counts (one round trip: a round's count loads issue back to back, one wait behind them) -> per
// segment SEG / BATCH slab round trips -> LDS, barrier -> wave 0: RED_ROUND / BATCH LDS round trips -> G (and W). Nothing in
// it lives in scratch.
template <int BATCH>
__global__ __launch_bounds__(RED_THREADS, BATCH == 16 ? 4 : 8) void reduce_kernel(const ReduceArgs R) {
    constexpr int C = RED_C, GPW = RED_GPW;
    __shared__ float4 s_T[RED_ROUND][C];
    __shared__ int s_cnt[RED_ROUND];
    __shared__ int s_x[4][40];         // the commit rows' exchange area
    // leading workgroups (blockIdx.y < gridDim.y - n_vf): one env row each — commit + next order
    const int sy_rows = (int)gridDim.y - R.n_vf;             // the commit rows come first in dispatch order
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    RED_STAMP(0);
    if ((int)blockIdx.y < sy_rows) {
        const int row = (int)blockIdx.y * (int)gridDim.x + blockIdx.x;      // one row per workgroup (waves 0..3): a row
        commit_and_place_row(R, row, wave, threadIdx.x & 63, s_x);          // moves ~25 KB, so spread them over the CUs
        if (wave < 4) RED_STAMP_DRAINED(1 + wave);
        return;
    }
    const int k = (int)blockIdx.y - sy_rows;
    // slab addresses = wave-uniform base (block, value function: SGPRs) + this lane's offset (one VGPR: its column and
    // its group's segment): sixteen 64-bit per-lane pointers would not fit beside the sixteen float4 in flight (the kernel ran at
    // the 128-VGPR cap with 8 spilled registers and a vmcnt(0) in front of the first slab load)
    const size_t slab_stride = (size_t)R.n_vf * RED_COLS * sizeof(float4);
    const char *slab_k = reinterpret_cast<const char *>(R.slabs) + (size_t)k * RED_COLS * sizeof(float4);
    const int nseg = (R.nblk + SEG - 1) / SEG;
    float4 S = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int nk = 0;                                                 // (wave-uniform)
    // wave 0 applies the update at the end: its W and scale columns are fetched under the last round's barrier
    float4 w_old = make_float4(0.0f, 0.0f, 0.0f, 0.0f), sc = w_old;
    int step_failed = 0;
    // A round = RED_SPW segments per lane group (32 segments = 512 blocks in all at RED_SPW = 2): the counts of all of a group's
    // segments are read first, then segment after segment its <= 16 slabs, BATCH loads in flight, and one barrier pair per round
    // (round 2: a round was one segment per wave — two dependent count -> slab round trips and two barrier pairs at 512 blocks)
    for (int sg0 = 0; sg0 < nseg; sg0 += RED_ROUND) {
        const int lane = lane_now();
        const int grp = wave * GPW + lane / C;      // this lane's group of the workgroup
        int cs[RED_SPW];
#pragma unroll
        for (int j = 0; j < RED_SPW; ++j) {
            // lane 16 r + l reads block b0 + l's count (every row of a group reads the same sixteen words); the load itself is
            // unconditional — a block past the end reads the last block's — and what it brings is dropped below: no branch between
            // the two loads (32-bit index: nblk * n_vf is small; the 64-bit form was hoisted and spilled)
            const int bl = (sg0 + j * RED_GROUPS + grp) * SEG + (lane & (SEG - 1));
            cs[j] = R.cnts[(unsigned)(min(bl, R.nblk - 1) * R.n_vf + k)];
        }
#pragma unroll
        for (int j = 0; j < RED_SPW; ++j) {
            const int b0w = (sg0 + j * RED_GROUPS + wave * GPW) * SEG;       // first block of the wave's first group (uniform)
            const int c = ((sg0 + j * RED_GROUPS + grp) * SEG + (lane & (SEG - 1)) < R.nblk) ? cs[j] : 0;
            const uint64_t ball = __ballot(c > 0);               // row r: which blocks of its group's segment hold a slab
            unsigned mask, any;                                  // this group's blocks; the blocks of any group of the wave (uniform)
            static_assert(C == 16, "a lane group is a row of 16 lanes: its blocks are its row's bits of the ballot");
            mask = (unsigned)(ball >> (lane & 48)) & 0xffffu;
            any = (unsigned)(ball | (ball >> 16) | (ball >> 32) | (ball >> 48)) & 0xffffu;
            float4 T = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (any) {
                // buffer loads: descriptor = the wave's first slab of this pass and value function (SGPRs), scalar offset = slab u,
                // vector offset = the lane's column and its group's segment (< 4 * 16 slabs: far below 2^31)
                const __amdgpu_buffer_rsrc_t seg = __builtin_amdgcn_make_buffer_rsrc(
                    const_cast<char *>(slab_k + (size_t)b0w * slab_stride), 0, 0x7fffffff, 0x00020000);
                const int i4 = blockIdx.x * C + (lane & (C - 1));
                unsigned col_off = (unsigned)(i4 < RED_COLS ? i4 : 0) * (unsigned)sizeof(float4);
                col_off += (unsigned)(lane / C) * (unsigned)(SEG * slab_stride);
#pragma unroll
                for (int h = 0; h < SEG; h += BATCH) {
                    if (!((any >> h) & ((1u << BATCH) - 1u))) continue;
                    u4v v[BATCH];
#pragma unroll
                    for (int u = 0; u < BATCH; ++u) {
                        v[u] = (u4v){0u, 0u, 0u, 0u};
                        if (!((any >> (h + u)) & 1u)) continue;
                        if ((mask >> (h + u)) & 1u) v[u] = __builtin_amdgcn_raw_buffer_load_b128(seg, (int)col_off, (int)((h + u) * (unsigned)slab_stride), 0);
                    }
#pragma unroll
                    for (int u = 0; u < BATCH; ++u) {
                        if ((any >> (h + u)) & 1u) {
                            T.x = T.x + __uint_as_float(v[u][0]); T.y = T.y + __uint_as_float(v[u][1]);
                            T.z = T.z + __uint_as_float(v[u][2]); T.w = T.w + __uint_as_float(v[u][3]);
                        }
                    }
                }
            }
            // Every slab load above has been waited for by its add; the compiler cannot see that (load and add hang on the same mask bit
            // in two branches) and would make wave 0 wait for W and scale, fetched below, in front of the second level's first LDS read,
            // where it reuses a load's registers. Said here, where it costs nothing.
            __builtin_amdgcn_s_waitcnt(0x0F70);                 // vmcnt(0)
            s_T[j * RED_GROUPS + grp][lane & (C - 1)] = T;      // (stored whether or not the segment holds a slab: an empty one's row is +0)
            const int ctot = row_sum(c);                        // (every row of a group holds its segment's sixteen counts)
            if ((lane & (C - 1)) == 0) s_cnt[j * RED_GROUPS + grp] = ctot;
        }
        const bool last = sg0 + RED_ROUND >= nseg;
        if (last) RED_STAMP(8 + wave);
        if (wave == 0 && last) RED_STAMP(5);
        if (wave == 0 && R.apply && last) {                     // last round: under the barrier and the second-level sum
            step_failed = *R.fail_flag;                         // (fetched with the weights; looked at where they would be written)
            const int ln = lane_now();
            const int i4 = blockIdx.x * C + (ln & (C - 1));       // (addresses made HERE: hoisted to the top of the kernel they are spilled)
            const int col = i4 < RED_COLS ? i4 : 0;
            w_old = reinterpret_cast<const float4 *>(R.W)[(size_t)k * RED_COLS + col];      // (not at the top of the kernel: held across the slab loads they were
            sc = *reinterpret_cast<const float4 *>(R.scale + (col * 4) % NF);     //  eight more registers — spilled at 64 VGPRs; NF % 4 == 0: no row straddling)
        }
        __syncthreads();
        if (wave == 0) {
            if (last) RED_STAMP(6);
            // The second level, segment order sg0 + u (SPEC §5), with no LDS latency in the add chain: the round's counts are read at
            // once, one per lane, and the rows of s_T BATCH at a time, every read of a batch issued before its first add (the
            // the lanes C.. read the columns of the lanes below them again; nothing of theirs is stored).
            // Every row is added, the empty segments' too. That gives the bits of the form that skips them:
            //   an empty segment's row is exactly +0 — T starts at +0, takes only +0 terms while the mask is 0, and is stored unconditionally;
            //   S starts at +0 and so never becomes -0: x + y is -0 only where x and y both are (round to nearest);
            //   therefore S + (+0) == S, bit for bit, for every value S can hold, Inf and NaN included.
            const int ln = lane_now();
            const int cl = ln & (C - 1);
            const int cu = row_sum(ln < RED_ROUND ? s_cnt[ln] : 0);       // rows 0 and 1 hold the 32 counts
            nk += __builtin_amdgcn_readlane(cu, 0) + __builtin_amdgcn_readlane(cu, 16);
#pragma unroll
            for (int h = 0; h < RED_ROUND; h += BATCH) {
                float4 t[BATCH];
#pragma unroll
                for (int u = 0; u < BATCH; ++u) t[u] = s_T[h + u][cl];
#pragma unroll
                for (int u = 0; u < BATCH; ++u) { S.x = S.x + t[u].x; S.y = S.y + t[u].y; S.z = S.z + t[u].z; S.w = S.w + t[u].w; }
            }
            if (last) RED_STAMP(7);
        }
        if (!last) __syncthreads();                             // (the next round parks its sums in the rows wave 0 has just read)
    }
    if (wave != 0) return;
    const int lane = lane_now(), i4 = blockIdx.x * C + lane;
    if (blockIdx.x == 0 && lane == 0) {
        R.n_k[k] = nk;
        if (R.nk_f) R.nk_f[k] = (float)nk;               // exact: counts stay far below 2^24
    }
    if (lane >= C || i4 >= RED_COLS) return;
    reinterpret_cast<float4 *>(R.G)[(size_t)k * RED_COLS + i4] = S;
    if (R.apply && nk > 0 && !step_failed) {       // (a step in which a workgroup gave up leaves W as it was)
        const float step = R.alpha / (float)max(nk, R.nk_floor);
        float4 w = w_old;
        w.x = fmaf(step * sc.x, S.x, w.x); w.y = fmaf(step * sc.y, S.y, w.y);
        w.z = fmaf(step * sc.z, S.z, w.z); w.w = fmaf(step * sc.w, S.w, w.w);
        reinterpret_cast<float4 *>(R.W)[(size_t)k * RED_COLS + i4] = w;
    }
    RED_STAMP_DRAINED(1);
}

// acting-only steps have no reduce launch: the commit alone, one workgroup of four waves per row of 256 envs
__global__ __launch_bounds__(256) void commit_kernel(const ReduceArgs R) {
    __shared__ int s_x[4][40];
    commit_and_place_row(R, blockIdx.x, threadIdx.x >> 6, threadIdx.x & 63, s_x);
}
