// scg_order.hpp — SPEC §5 env order: the sort key, the layout of the option runs over the workgroups (shared with the commit rows of
// scg_reduce_kernel.hpp) and the stand-alone counting sort (sort_hist_kernel, sort_scatter_kernel). Included by scg_kernels.hip.
#pragma once

// SPEC §5 env order from the key totals (all lanes compute the same few integers). Runs of the keys 1..6 follow one
// another in key order; envs of key 0 (running no option) are the filler:
//  * chunked layout (the normal case): every workgroup gets at most c envs of one option's run at its start and
//    key-0 envs behind them, with c = ceil(S / (full workgroups - non-empty runs)) — so the option work is spread
//    evenly over ALL workgroups instead of leaving the key-0 workgroups idle after their root pass (one workgroup
//    per CU: the launch lasts as long as its slowest), and no workgroup ever holds two options' runs (a third
//    pass). What is left of key 0 comes last.
//  * padded layout (when the option runs alone need more workgroups than there are full ones): runs back to back,
//    each padded with key-0 envs to the next workgroup boundary while any are left.
// floor(r / d) for r < 2^24, d <= 2^30, with m = ceil(2^32 / d) (m wraps to 0 for d = 1)
__device__ __forceinline__ uint32_t div_magic(uint32_t d) { return 0xFFFFFFFFu / d + 1u; }
__device__ __forceinline__ int div_by(int r, int d, uint32_t m) { return d == 1 ? r : (int)__umulhi((uint32_t)r, m); }
// SPEC §5 sort key of an env from its signed option id: k in [1, n_vf) (running option k) -> k; 0 and -k (no option in sight / inside
// option k's initiation set but staying out of it, §4.2: either way the env runs the root) -> 0; anything else -> the last key n_vf.
// NKEY keys, count tables with HSTRIDE ints per row.
constexpr int NKEY = 7, HSTRIDE = 8;
__device__ __forceinline__ int sort_key(int o, int n_vf) {
    if (o <= 0) return o > -n_vf ? 0 : n_vf;
    return o < n_vf ? o : n_vf;
}
struct OrderLayout {
    int chunked, c, g, U, Ftot;
    uint32_t mc, mg;               // ceil(2^32 / c), ceil(2^32 / g): exact division of ranks (< 2^24) by mul-high
    int start[NKEY];               // position of run k's first env
    int cnt[NKEY], n[NKEY], F[NKEY];   // chunked: workgroups of run k, its size, key-0 fill slots before it
    int pad_lo[NKEY], pad_n[NKEY], pad_pos[NKEY], tail_lo, tail_pos;     // padded layout
};
__device__ __forceinline__ void order_layout(const int tot[NKEY], int n_envs, OrderLayout &L) {
    int S = 0, Rn = 0;
#pragma unroll
    for (int k = 1; k < NKEY; ++k) { S += tot[k]; Rn += tot[k] > 0 ? 1 : 0; L.n[k] = tot[k]; }
    L.n[0] = tot[0];
    const int Bf = n_envs / BLOCK_ENVS;
    int c = BLOCK_ENVS;
    if (Bf > Rn && S > 0) c = min(BLOCK_ENVS, (S + (Bf - Rn) - 1) / (Bf - Rn));
    int U = 0, F = 0;
    L.start[0] = 0; L.cnt[0] = 0; L.F[0] = 0;
    L.mc = div_magic((uint32_t)c);
    L.mg = div_magic((uint32_t)max(BLOCK_ENVS - c, 1));
#pragma unroll
    for (int k = 1; k < NKEY; ++k) {
        L.cnt[k] = div_by(tot[k] + c - 1, c, L.mc);
        L.start[k] = U * BLOCK_ENVS; L.F[k] = F;
        U += L.cnt[k]; F += L.cnt[k] * BLOCK_ENVS - tot[k];
    }
    L.c = c; L.g = BLOCK_ENVS - c; L.U = U; L.Ftot = F;
    L.chunked = (U * BLOCK_ENVS <= n_envs) ? 1 : 0;
    if (!L.chunked) {
        int P = 0, used = 0;
        L.c = 1 << 30;                                  // one "chunk" per run: pos = start + rank
        L.mc = div_magic(1u << 30);
        L.pad_lo[0] = 0; L.pad_n[0] = 0; L.pad_pos[0] = 0;
#pragma unroll
        for (int k = 1; k < NKEY; ++k) {
            L.start[k] = P; P += tot[k];
            const int need = tot[k] > 0 ? (BLOCK_ENVS - P % BLOCK_ENVS) % BLOCK_ENVS : 0;
            const int pad = min(need, tot[0] - used);
            L.pad_lo[k] = used; L.pad_n[k] = pad; L.pad_pos[k] = P; used += pad; P += pad;
        }
        L.tail_lo = used; L.tail_pos = P;
    }
}
// position of the r-th env of run k (k >= 1; `start` = L.start[k] selected by the caller)
__device__ __forceinline__ int order_posk(const OrderLayout &L, int start, int r) {
    const int t = div_by(r, L.c, L.mc);
    return start + BLOCK_ENVS * t + (r - t * L.c);
}
__device__ __forceinline__ int order_pos0(const OrderLayout &L, int r) {       // position of the r-th key-0 env
    if (!L.chunked) {
        int pos = L.tail_pos + (r - L.tail_lo);
#pragma unroll
        for (int k = 1; k < NKEY; ++k)
            if (r >= L.pad_lo[k] && r < L.pad_lo[k] + L.pad_n[k]) pos = L.pad_pos[k] + (r - L.pad_lo[k]);
        return pos;
    }
    int pos = L.U * BLOCK_ENVS + (r - L.Ftot);          // behind all runs
    int st = 0, cn = 0, nk = 0, f0 = 0;
    bool in_run = false;
#pragma unroll
    for (int k = 1; k < NKEY; ++k) {
        const int fills = L.cnt[k] * BLOCK_ENVS - L.n[k];
        if (r >= L.F[k] && r < L.F[k] + fills) { in_run = true; st = L.start[k]; cn = L.cnt[k]; nk = L.n[k]; f0 = L.F[k]; }
    }
    if (in_run) {
        const int rp = r - f0, nfull = cn - 1;
        if (L.g > 0 && rp < nfull * L.g) {
            const int t = div_by(rp, L.g, L.mg);
            pos = st + BLOCK_ENVS * t + L.c + (rp - t * L.g);
        } else {
            pos = st + BLOCK_ENVS * nfull + (nk - nfull * L.c) + (rp - nfull * L.g);
        }
    }
    return pos;
}

// SPEC §5 env order: stable counting sort of the envs by option_id (6 keys), two tiny kernels per step.
// Option-homogeneous workgroups turn five sparse option passes per workgroup into about one dense one.
__global__ __launch_bounds__(256) void sort_hist_kernel(const int32_t *option_id, int n, int n_vf, int32_t *hist) {
    __shared__ int s_c[4][HSTRIDE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e = blockIdx.x * 256 + tid;
    const int o = e < n ? sort_key(option_id[e], n_vf) : -1;          // (out-of-range ids sort last)
#pragma unroll
    for (int k = 0; k < NKEY; ++k) {
        const uint64_t m = __ballot(o == k);
        if (lane == 0) s_c[wave][k] = __popcll(m);
    }
    __syncthreads();
    if (tid < NKEY) hist[blockIdx.x * HSTRIDE + tid] = s_c[0][tid] + s_c[1][tid] + s_c[2][tid] + s_c[3][tid];
}

__global__ __launch_bounds__(256) void sort_scatter_kernel(const int32_t *option_id, int n, int n_vf, int nblk,
                                                           const int32_t *hist, int32_t *perm, int32_t *invperm) {
    __shared__ int s_c[4][HSTRIDE];
    __shared__ int s_off[HSTRIDE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    // offset of (key k, block b) in the sorted order = (all envs with a smaller key) + (key-k envs of earlier blocks)
    __shared__ int s_tot[HSTRIDE], s_pre[HSTRIDE], s_part[4][2 * HSTRIDE];
    int tot[NKEY], pre[NKEY];
#pragma unroll
    for (int kk = 0; kk < NKEY; ++kk) { tot[kk] = 0; pre[kk] = 0; }
    for (int bb0 = 0; bb0 < nblk; bb0 += 256) {
        const int bb = bb0 + tid;
        if (bb < nblk) {
#pragma unroll
            for (int kk = 0; kk < NKEY; ++kk) {
                const int h = hist[bb * HSTRIDE + kk];
                tot[kk] += h;
                if (bb < b) pre[kk] += h;
            }
        }
    }
#pragma unroll
    for (int kk = 0; kk < NKEY; ++kk) {                       // integer sums: any order
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) { tot[kk] += __shfl_xor(tot[kk], m, 64); pre[kk] += __shfl_xor(pre[kk], m, 64); }
        if (lane == 0) { s_part[wave][kk] = tot[kk]; s_part[wave][HSTRIDE + kk] = pre[kk]; }
    }
    __syncthreads();
    if (tid < NKEY) {
        s_tot[tid] = s_part[0][tid] + s_part[1][tid] + s_part[2][tid] + s_part[3][tid];
        s_pre[tid] = s_part[0][HSTRIDE + tid] + s_part[1][HSTRIDE + tid] + s_part[2][HSTRIDE + tid] + s_part[3][HSTRIDE + tid];
    }
    __syncthreads();
    int tt[NKEY];
#pragma unroll
    for (int kk = 0; kk < NKEY; ++kk) tt[kk] = s_tot[kk];
    OrderLayout L;
    order_layout(tt, n, L);
    if (tid < NKEY) s_off[tid] = s_pre[tid];               // rank of the row's first key-k env within its run
    const int e = b * 256 + tid;
    const int o = e < n ? sort_key(option_id[e], n_vf) : -1;
    int rank = 0;
#pragma unroll
    for (int k = 0; k < NKEY; ++k) {
        const uint64_t m = __ballot(o == k);
        if (lane == 0) s_c[wave][k] = __popcll(m);
        if (o == k) rank = __popcll(m & ((1ull << lane) - 1ull));
    }
    __syncthreads();
    if (o >= 0) {
        int rk = s_off[o] + rank;
        for (int w = 0; w < wave; ++w) rk += s_c[w][o];
        int st = 0;
#pragma unroll
        for (int k = 1; k < NKEY; ++k) if (o == k) st = L.start[k];
        const int pos = o == 0 ? order_pos0(L, rk) : order_posk(L, st, rk);
        perm[pos] = e;
        invperm[e] = pos;
    }
}
