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
    const float4 *qalt;            // the root's Q(s', .) of the envs whose result line carries the declined mark (SPEC §4.2)
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
constexpr int RED_WAVES = 16;      // one wave per segment, 16 segments per round
constexpr int RED_THREADS = 64 * RED_WAVES;
constexpr int RED_SPW = 2;         // segments per wave and round
constexpr int RED_COLS = NACT * NF / 4;                              // float4 columns per value function
constexpr int RED_NCOL = (RED_COLS + 63) / 64;
constexpr int RED_STAMP_SLOTS = 8;  // diagnostic build: [0] entry, [1] exit (row workgroups: [1..4] = waves 0..3), slab wave 0: [5] sums parked, [6] barrier passed, [7] G summed

// Four waves per row of 256 envs (wave wv owns envs 64 wv .. 64 wv + 63 of the row), two dependent memory round trips
// and one workgroup barrier in all:
//   commit: gather each env's result line from its position in the current order (one 64-byte read) and write
//           the caller's SoA arrays (state, outputs, qcache) with full-line stores;
//   sort  : place the row in the stable counting-sort order of the next step (7 keys), from the per-row key
//           counts of all rows: offset(key k, row) = (envs with a smaller key) + (key-k envs of earlier rows)
//           (+ key-k envs of the row's earlier waves, exchanged through LDS together with the waves' shares of the
//           count table).
// Every thread of the workgroup must call this (it holds the barrier); waves >= 4 only pass through it.
// Load order matters: position first, then the count table, then the record, so that the table's latency hides
// under the record's and the prefix sums run while the record is in flight. One wave per row (four envs per lane)
// took 8.3 us of dependent work after the launch floor; see DESIGN §10.
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
    const int pos_old = ok ? R.invperm[e] : 0;
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
    float4 ra = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rb = ra, rq = ra;
    float q4 = 0.0f;
    if (ok) {
        const float4 *r = R.outrec + (size_t)pos_old * OREC;
        const float4 r3 = r[3];
        ra = r[0]; rb = r[1]; rq = r[2]; q4 = r3.x;
        if (__float_as_uint(r3.y) == OREC_DECLINED) {       // SPEC §4.2: the option promised less than the root — the env stays with the root
            rq = R.qalt[(size_t)pos_old * 2]; q4 = R.qalt[(size_t)pos_old * 2 + 1].x;
            rb.y = __uint_as_float(__float_as_uint(rb.y) | 0x01000000u);      // declined: bit 24 of the record's bits
        }
    }
    int key = -1;
    uint64_t km[NKEY];
    if (act) {
        if (R.sort) {
#pragma unroll
            for (int k = 0; k < NKEY; ++k) {                   // integer sums: any order
#pragma unroll
                for (int m = 1; m < 64; m <<= 1) { tot[k] += __shfl_xor(tot[k], m, 64); pre[k] += __shfl_xor(pre[k], m, 64); }
            }
        }
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
                int v = 0;
#pragma unroll
                for (int k = 0; k < NKEY; ++k) {
                    if (lane == k) v = tot[k];
                    if (lane == NKEY + k) v = pre[k];
                    if (lane == 2 * NKEY + k) v = __popcll(km[k]);
                }
                s_x[wv][lane] = v;
            }
        }
    }
    if (R.c_rows && act) {                                  // the announced trigger's examples of this wave's envs (SPEC §7)
        bool in;
        int v = collect_v(e, R.n, R.c_events, R.c_prev, R.c_bits, R.c_evlen, R.c_ring_len, R.c_L, in);
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
        if (lane == 0) s_x[wv][3 * NKEY] = v;
    }
    if (!R.sort && !R.c_rows) return;                       // workgroup-uniform
    __syncthreads();
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

// diagnostic build (make rstamps; tools/reduce_chain.py): every workgroup leaves the 100 MHz clock at entry, at exit and, in the slab
// half, at wave 0's steps in between. Not in the product: the macro is empty and ReduceArgs has no such field.
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

// grid (column chunks, n_vf [+ rows of the env order]). A workgroup owns 64 float4 columns of one value function;
// its 16 waves each sum one segment's slabs, T_s = ((P_16s + P_16s+1) + ...) over the non-empty blocks with BATCH
// loads in flight, park T_s in LDS, and wave 0 adds the segments in order, G = ((T_0 + T_1) + ...)
// — SPEC §5's two levels in one launch.
// BATCH = slab loads in flight per wave: 16 (one 16-wave workgroup per CU: one memory round trip per segment — for launches
// whose workgroups fit the chip in one round anyway) or 8 (64 VGPRs, two workgroups per CU: the bench size's workgroups are resident
// together instead of in two rounds). The sum runs in block order either way: same bits.
// A slab workgroup's chain is: the counts (one round trip: a round's count loads issue back to back, one wait behind them) -> per
// segment SEG / BATCH slab round trips -> LDS, barrier -> wave 0: RED_WAVES * RED_SPW / BATCH LDS round trips -> G (and W). Nothing in
// it lives in scratch.
template <int BATCH>
__global__ __launch_bounds__(RED_THREADS, BATCH == 16 ? 4 : 8) void reduce_kernel(const ReduceArgs R) {
    __shared__ float4 s_T[RED_WAVES * RED_SPW][64];
    __shared__ int s_cnt[RED_WAVES * RED_SPW];
    __shared__ int s_x[4][40];         // the commit rows' exchange area
    // leading workgroups (blockIdx.y < gridDim.y - n_vf): one env row each — commit + next order
    const int sy_rows = (int)gridDim.y - R.n_vf;             // the commit rows come FIRST in dispatch order (round 5: theirs was the longer chain. By round 15's stamps
                                                             //  the root's slab workgroups, which start 0.4 us behind them, end the launch; the other order is untried)
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    RED_STAMP(0);
    if ((int)blockIdx.y < sy_rows) {
        const int row = (int)blockIdx.y * (int)gridDim.x + blockIdx.x;      // one row per workgroup (waves 0..3): a row
        commit_and_place_row(R, row, wave, threadIdx.x & 63, s_x);          // moves ~25 KB, so spread them over the CUs
        if (wave < 4) RED_STAMP_DRAINED(1 + wave);
        return;
    }
    const int k = (int)blockIdx.y - sy_rows;
    // slab addresses = wave-uniform base (block, value function: SGPRs) + this lane's column offset (one VGPR): sixteen
    // 64-bit per-lane pointers would not fit beside the sixteen float4 in flight (the kernel ran at the 128-VGPR cap
    // with 8 spilled registers and a vmcnt(0) in front of the first slab load)
    const size_t slab_stride = (size_t)R.n_vf * RED_COLS * sizeof(float4);
    const char *slab_k = reinterpret_cast<const char *>(R.slabs) + (size_t)k * RED_COLS * sizeof(float4);
    const int nseg = (R.nblk + SEG - 1) / SEG;
    float4 S = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int nk = 0;                                                 // (wave-uniform)
    // wave 0 applies the update at the end: its W and scale columns are fetched under the last round's barrier
    float4 w_old = make_float4(0.0f, 0.0f, 0.0f, 0.0f), sc = w_old;
    int step_failed = 0;
    // A round = RED_SPW segments per wave (32 segments = 512 blocks in all at RED_SPW = 2): the counts of all of a wave's segments are
    // read first, then segment after segment its <= 16 slabs, BATCH loads in flight, and one barrier pair per round (round 2: a round
    // was one segment per wave — two dependent count -> slab round trips and two barrier pairs at 512 blocks)
    for (int sg0 = 0; sg0 < nseg; sg0 += RED_WAVES * RED_SPW) {
        const int lane = lane_now();
        int cs[RED_SPW];
#pragma unroll
        for (int j = 0; j < RED_SPW; ++j) {
            // lane l < 16 reads block b0 + l's count; the load itself is unconditional — lanes 16..63 read lanes 0..15's words again, a
            // block past the end reads the last block's — and what it brings is dropped below: no branch between the two loads
            // (32-bit index: nblk * n_vf is small; the 64-bit form was hoisted and spilled)
            const int bl = (sg0 + j * RED_WAVES + wave) * SEG + (lane & (SEG - 1));
            cs[j] = R.cnts[(unsigned)(min(bl, R.nblk - 1) * R.n_vf + k)];
        }
#pragma unroll
        for (int j = 0; j < RED_SPW; ++j) {
            const int b0 = (sg0 + j * RED_WAVES + wave) * SEG;
            const int c = (lane < SEG && b0 + lane < R.nblk) ? cs[j] : 0;
            const unsigned mask = (unsigned)__ballot(c > 0);     // wave-uniform: which of the segment's blocks hold a slab
            float4 T = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (mask) {
                // buffer loads: descriptor = the segment's first slab of this value function (SGPRs), scalar offset = slab u,
                // vector offset = the lane's column
                const __amdgpu_buffer_rsrc_t seg = __builtin_amdgcn_make_buffer_rsrc(
                    const_cast<char *>(slab_k + (size_t)b0 * slab_stride), 0, 0x7fffffff, 0x00020000);
                const int i4 = blockIdx.x * 64 + lane;
                const unsigned col_off = (unsigned)(i4 < RED_COLS ? i4 : 0) * (unsigned)sizeof(float4);
#pragma unroll
                for (int h = 0; h < SEG; h += BATCH) {
                    if (!((mask >> h) & ((1u << BATCH) - 1u))) continue;
                    u4v v[BATCH];
#pragma unroll
                    for (int u = 0; u < BATCH; ++u) {
                        v[u] = (u4v){0u, 0u, 0u, 0u};
                        if ((mask >> (h + u)) & 1u) v[u] = __builtin_amdgcn_raw_buffer_load_b128(seg, (int)col_off, (int)((h + u) * (unsigned)slab_stride), 0);
                    }
#pragma unroll
                    for (int u = 0; u < BATCH; ++u) {
                        if ((mask >> (h + u)) & 1u) {
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
            s_T[j * RED_WAVES + wave][lane] = T;                 // (stored whether or not the segment holds a slab: an empty one's row is +0)
            const int ctot = row_sum(c);                        // (lanes 0..15 are row 0)
            if (lane == 0) s_cnt[j * RED_WAVES + wave] = ctot;
        }
        const bool last = sg0 + RED_WAVES * RED_SPW >= nseg;
        if (wave == 0 && last) RED_STAMP(5);
        if (wave == 0 && R.apply && last) {                     // last round: under the barrier and the second-level sum
            step_failed = *R.fail_flag;                         // (fetched with the weights; looked at where they would be written)
            const int i4 = blockIdx.x * 64 + lane_now();        // (addresses made HERE: hoisted to the top of the kernel they are spilled)
            const int col = i4 < RED_COLS ? i4 : 0;
            w_old = reinterpret_cast<const float4 *>(R.W)[(size_t)k * RED_COLS + col];      // (not at the top of the kernel: held across the slab loads they were
            sc = *reinterpret_cast<const float4 *>(R.scale + (col * 4) % NF);     //  eight more registers — spilled at 64 VGPRs; NF % 4 == 0: no row straddling)
        }
        __syncthreads();
        if (wave == 0) {
            if (last) RED_STAMP(6);
            // The second level, segment order sg0 + u (SPEC §5), with no LDS latency in the add chain: the round's counts are read at
            // once, one per lane, and the rows of s_T BATCH at a time, every read of a batch issued before its first add.
            // Every row is added, the empty segments' too. That gives the bits of the form that skips them:
            //   an empty segment's row is exactly +0 — T starts at +0, is not touched while the mask is 0, and is stored unconditionally;
            //   S starts at +0 and so never becomes -0: x + y is -0 only where x and y both are (round to nearest);
            //   therefore S + (+0) == S, bit for bit, for every value S can hold, Inf and NaN included.
            const int ln = lane_now();
            const int cu = row_sum(ln < RED_WAVES * RED_SPW ? s_cnt[ln] : 0);       // rows 0 and 1 hold the 32 counts
            nk += __builtin_amdgcn_readlane(cu, 0) + __builtin_amdgcn_readlane(cu, 16);
#pragma unroll
            for (int h = 0; h < RED_WAVES * RED_SPW; h += BATCH) {
                float4 t[BATCH];
#pragma unroll
                for (int u = 0; u < BATCH; ++u) t[u] = s_T[h + u][ln];
#pragma unroll
                for (int u = 0; u < BATCH; ++u) { S.x = S.x + t[u].x; S.y = S.y + t[u].y; S.z = S.z + t[u].z; S.w = S.w + t[u].w; }
            }
            if (last) RED_STAMP(7);
        }
        if (!last) __syncthreads();                             // (the next round parks its sums in the rows wave 0 has just read)
    }
    if (wave != 0) return;
    const int lane = lane_now(), i4 = blockIdx.x * 64 + lane;
    if (blockIdx.x == 0 && lane == 0) {
        R.n_k[k] = nk;
        if (R.nk_f) R.nk_f[k] = (float)nk;               // exact: counts stay far below 2^24
    }
    if (i4 >= RED_COLS) return;
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
