// scg_collect_kernels.hpp — SPEC §7 / §13 example collection from the trajectory ring: harvest_kernel, the device-side trigger
// (collect_count_kernel, collect_scatter_kernel) and the frontier collection per node of the skill graph (frontier_count_kernel,
// frontier_scatter_kernel). Included by scg_kernels.hip in front of scg_reduce_kernel.hpp, whose commit rows use collect_v.
#pragma once

// SPEC §7: examples for an initiation-set fit, gathered from the trajectory ring (one thread per example)
__global__ __launch_bounds__(256) void harvest_kernel(int n_sel, const int32_t *sel_env, const float *ring_x,
                                                      const float *ring_y, int ring_len, int n, const int32_t *ev_len,
                                                      int l_pos, int l_neg, float *out_xy, uint8_t *out_label) {
    const int L = l_pos + l_neg;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)n_sel * L) return;
    const int si = (int)(t / L), j = (int)(t - (long long)si * L);       // j = age: 0 = most recent recorded state
    const int e = sel_env[si];
    const int idx = ev_len[e] - 1 - j;
    const bool ok = idx >= 0 && j < ring_len;
    float x = 0.0f, y = 0.0f;
    if (ok) {
        const size_t row = (size_t)(idx & (ring_len - 1)) * n + e;
        x = ring_x[row]; y = ring_y[row];
    }
    out_xy[2 * t] = x; out_xy[2 * t + 1] = y;
    out_label[t] = ok ? (j < l_pos ? 1 : 0) : 255;
}

// SPEC §7 device-side trigger + harvest (no host round trip per step), two small launches over rows of COL_ROW envs — or one,
// when the trigger was announced with scg_arm_collect: the commit rows of the step's own last launch then leave the row totals.
// An env is selected when (events & bits) != 0 — with `prev_in` given, only on the step it ENTERS that state (prev_in is
// updated). A selected env contributes its v = min(L, ev_len, ring_len) most recent ring states (age j < l_pos: label 1,
// else 0), appended behind the *count examples the buffer already holds, in env order, ages ascending; what does not fit
// into `cap` is dropped.
//   collect_count_kernel    row totals of v (integer sums: order-free) -> rowsum[row]; the buffer's fill level -> rowsum[nrows]
//   collect_scatter_kernel  offset of a row = fill level + totals of the rows before it; inside a row ballots + popcounts
//                           per wave and a 16-entry scan across the waves; a selected env's examples are gathered by the
//                           lanes of its wave together (lane j = age j), not one after another by the env's own lane
// Deterministic: every position is a prefix sum of integers in env order. (Round 2 walked the envs with ONE workgroup,
// 1024 at a time behind three barriers each: 64 dependent memory round trips per step-batch at the bench size.)
constexpr int COL_ROW = 256;                   // = the env rows of the commit workgroups, which can stand in for collect_count_kernel

__device__ __forceinline__ int collect_v(int e, int n, const uint8_t *events, const uint8_t *prev_in, uint32_t bits,
                                         const int32_t *ev_len, int ring_len, int L, bool &in_out) {
    in_out = false;
    if (e >= n) return 0;
    const bool in = (events[e] & bits) != 0;
    in_out = in;
    const bool hit = prev_in ? (in && !prev_in[e]) : in;
    return hit ? min(min(L, ev_len[e]), ring_len) : 0;
}

__global__ __launch_bounds__(COL_ROW) void collect_count_kernel(int n, const uint8_t *events, const uint8_t *prev_in,
                                                                uint32_t bits, const int32_t *ev_len, int ring_len, int L,
                                                                int32_t *rowsum, int nrows, const int32_t *count) {
    __shared__ int s_w[COL_ROW / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    bool in;
    int v = collect_v(blockIdx.x * COL_ROW + tid, n, events, prev_in, bits, ev_len, ring_len, L, in);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    if (lane == 0) s_w[wave] = v;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
#pragma unroll
        for (int w2 = 0; w2 < COL_ROW / 64; ++w2) t += s_w[w2];
        rowsum[blockIdx.x] = t;
        if (blockIdx.x == 0) rowsum[nrows] = *count;
    }
}

// One row's examples of one buffer, for both scatter kernels. Thread `e` of the row holds v examples (ev_len[e] = evl); `rowsum` is the
// buffer's row of totals (fill level at [nrows]); s_w / s_pre / s_tot have one slot per wave. Every thread of the workgroup must call
// this (it holds the barrier).
__device__ __forceinline__ void scatter_row(int v, int evl, int e, int n, const int32_t *rowsum, int nrows, const float *ring_x,
                                            const float *ring_y, int ring_len, int l_pos, float *ex_xy, uint8_t *ex_label,
                                            int32_t *count, int cap, int *s_w, int *s_pre, int *s_tot) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = blockIdx.x;
    // totals of the rows before this one (and of all rows, for the new fill level)
    int before = 0, all = 0;
    for (int r = tid; r < nrows; r += COL_ROW) { const int t = rowsum[r]; all += t; if (r < row) before += t; }
    int incl = v;                                          // inclusive prefix of v inside the wave
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const int t = __shfl_up(incl, m, 64);
        if (lane >= m) incl += t;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) { before += __shfl_xor(before, m, 64); all += __shfl_xor(all, m, 64); }
    if (lane == 63) s_w[wave] = incl;
    if (lane == 0) { s_pre[wave] = before; s_tot[wave] = all; }
    __syncthreads();
    int base = rowsum[nrows], woff = 0, total = 0;
#pragma unroll
    for (int w2 = 0; w2 < COL_ROW / 64; ++w2) {
        base += s_pre[w2]; total += s_tot[w2];
        if (w2 < wave) woff += s_w[w2];
    }
    if (row == 0 && tid == 0) *count = min(rowsum[nrows] + total, cap);
    const int pos0 = base + woff + incl - v;
    // the wave's selected envs one after another, the examples of one env on as many lanes
    uint64_t hits = __ballot(v > 0);
    while (hits) {
        const int src = (int)__builtin_ctzll(hits);
        hits &= hits - 1;
        const int he = __shfl(e, src, 64), hv = __shfl(v, src, 64), hp = __shfl(pos0, src, 64), hl = __shfl(evl, src, 64);
        for (int j = lane; j < hv; j += 64) {
            const int pos = hp + j;
            if ((unsigned)pos < (unsigned)cap) {            // (a negative fill level handed in writes nothing in front of the buffer)
                const size_t rrow = (size_t)((hl - 1 - j) & (ring_len - 1)) * n + he;
                ex_xy[2 * (size_t)pos] = ring_x[rrow]; ex_xy[2 * (size_t)pos + 1] = ring_y[rrow];
                ex_label[pos] = j < l_pos ? 1 : 0;
            }
        }
    }
}

__global__ __launch_bounds__(COL_ROW) void collect_scatter_kernel(int n, const uint8_t *events, uint8_t *prev_in, uint32_t bits,
                                                                  const float *ring_x, const float *ring_y, int ring_len,
                                                                  const int32_t *ev_len, int l_pos, int l_neg, float *ex_xy,
                                                                  uint8_t *ex_label, int32_t *count, int cap,
                                                                  const int32_t *rowsum, int nrows) {
    __shared__ int s_w[COL_ROW / 64], s_pre[COL_ROW / 64], s_tot[COL_ROW / 64];
    const int tid = threadIdx.x, L = l_pos + l_neg;
    const int e = blockIdx.x * COL_ROW + tid;
    bool in;
    const int v = collect_v(e, n, events, prev_in, bits, ev_len, ring_len, L, in);
    const int evl = v > 0 ? ev_len[e] : 0;
    if (prev_in && e < n) prev_in[e] = in ? 1 : 0;        // only this thread reads or writes this byte in this launch
    scatter_row(v, evl, e, n, rowsum, nrows, ring_x, ring_y, ring_len, l_pos, ex_xy, ex_label, count, cap, s_w, s_pre, s_tot);
}

// SPEC §13 frontier collection: §7's collect with one example buffer per node of the skill graph (node 0 = the goal, events
// bit 0; node p >= 1 = initiation set p, events bit p) and a stateless entry test in place of prev_in: an env hits node p when
// p is a target, its step ended in node p, and s_t (ring[(ev_len - 1) & (ring_len - 1)], harvest age 0) lies in no set of
// cover_mask (§4.1's z, no `known` term). The same two launches over rows of COL_ROW envs as collect_*_kernel:
//   frontier_count_kernel    per-row totals of v PER NODE -> rowsum[p][row]; node p's fill level -> rowsum[p][nrows]
//   frontier_scatter_kernel  node by node: offset of a row = fill level + totals of the rows before it, ballots + scans per
//                            wave, the hit env's rows gathered by the lanes of its wave (lane j = age j)
// Integer prefix sums in env order only; the classifier rows are staged in LDS once per workgroup; s_t is read once per env
// (and only for an env whose step ended in a target node).
__device__ __forceinline__ uint32_t frontier_hits(int e, int n, const uint8_t *events, const int32_t *ev_len, const float *ring_x,
                                                  const float *ring_y, int ring_len, const float *s_clf, uint32_t target_mask,
                                                  uint32_t cover_mask, int L, int &v, int &evl) {
    v = 0; evl = 0;
    if (e >= n) return 0u;
    const uint32_t cand = events[e] & target_mask;
    if (!cand) return 0u;
    const int el = ev_len[e];
    if (el < 1) return 0u;
    const size_t row = (size_t)((el - 1) & (ring_len - 1)) * n + e;
    const float x = ring_x[row], y = ring_y[row];
    for (uint32_t m = cover_mask; m; m &= m - 1)
        if (clf_z(s_clf + CLF_STRIDE * __builtin_ctz(m), x, y) > 0.0f) return 0u;     // s_t is covered: not an entry
    v = min(min(L, el), ring_len);
    evl = el;
    return cand;
}

__global__ __launch_bounds__(COL_ROW) void frontier_count_kernel(int n, const uint8_t *events, const int32_t *ev_len,
                                                                 const float *ring_x, const float *ring_y, int ring_len,
                                                                 const float *clf, int n_vf, uint32_t target_mask,
                                                                 uint32_t cover_mask, int L, int32_t *rowsum, int nrows,
                                                                 const int32_t *count) {
    __shared__ float s_clf[MAX_VF * CLF_STRIDE];
    __shared__ int s_w[MAX_VF][COL_ROW / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < n_vf * CLF_STRIDE) s_clf[tid] = clf[tid];
    __syncthreads();
    int v, evl;
    const uint32_t hit = frontier_hits(blockIdx.x * COL_ROW + tid, n, events, ev_len, ring_x, ring_y, ring_len, s_clf,
                                       target_mask, cover_mask, L, v, evl);
#pragma unroll
    for (int p = 0; p < MAX_VF; ++p) {
        if (!((target_mask >> p) & 1u)) continue;
        int vp = ((hit >> p) & 1u) ? v : 0;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) vp += __shfl_xor(vp, m, 64);
        if (lane == 0) s_w[p][wave] = vp;
    }
    __syncthreads();
    if (tid < MAX_VF && ((target_mask >> tid) & 1u)) {
        int t = 0;
#pragma unroll
        for (int w2 = 0; w2 < COL_ROW / 64; ++w2) t += s_w[tid][w2];
        rowsum[(size_t)tid * (nrows + 1) + blockIdx.x] = t;
        if (blockIdx.x == 0) rowsum[(size_t)tid * (nrows + 1) + nrows] = count[tid];
    }
}

__global__ __launch_bounds__(COL_ROW) void frontier_scatter_kernel(int n, const uint8_t *events, const int32_t *ev_len,
                                                                   const float *ring_x, const float *ring_y, int ring_len,
                                                                   const float *clf, int n_vf, uint32_t target_mask,
                                                                   uint32_t cover_mask, int l_pos, int l_neg, float *ex_xy,
                                                                   uint8_t *ex_label, int32_t *count, int cap,
                                                                   const int32_t *rowsum, int nrows) {
    __shared__ float s_clf[MAX_VF * CLF_STRIDE];
    __shared__ int s_w[MAX_VF][COL_ROW / 64], s_pre[MAX_VF][COL_ROW / 64], s_tot[MAX_VF][COL_ROW / 64];
    const int tid = threadIdx.x;
    if (tid < n_vf * CLF_STRIDE) s_clf[tid] = clf[tid];
    __syncthreads();
    const int e = blockIdx.x * COL_ROW + tid;
    int v, evl;
    const uint32_t hit = frontier_hits(e, n, events, ev_len, ring_x, ring_y, ring_len, s_clf, target_mask, cover_mask,
                                       l_pos + l_neg, v, evl);
    for (int p = 0; p < n_vf; ++p) {                      // uniform over the workgroup: scatter_row's barrier is reached by all
        if (!((target_mask >> p) & 1u)) continue;                // (each node has its own LDS slots: no barrier before the next node's writes)
        scatter_row(((hit >> p) & 1u) ? v : 0, evl, e, n, rowsum + (size_t)p * (nrows + 1), nrows, ring_x, ring_y, ring_len, l_pos,
                    ex_xy + (size_t)p * cap * 2, ex_label + (size_t)p * cap, count + p, cap, s_w[p], s_pre[p], s_tot[p]);
    }
}
