// scg_apply_kernels.hpp — SPEC §5's update W += alpha / n_k * scale * G outside the reduce launch: from one operand (apply_kernel), from
// the ranks' operands in slot order (apply_slots_kernel), and over the peer transport (peer_publish_kernel, peer_wait_kernel,
// apply_peers_kernel). Included by scg_kernels.hip.
#pragma once

// One weight's update: a value function without an update in the batch (n_k = 0) keeps its row; `scale_f` = the weight's column scale
__device__ __forceinline__ void apply_weight(float *w, float g, int nk, const float *scale_f, float alpha, int nk_floor) {
    if (nk <= 0) return;
    const float step = alpha / (float)max(nk, nk_floor);
    *w = fmaf(step * *scale_f, g, *w);
}

__global__ __launch_bounds__(256) void apply_kernel(float *W, const float *G, const int32_t *n_k, const float *nk_f,
                                                    const float *scale, float alpha, int nk_floor) {
    const int k = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= NACT * NF) return;
    const int nk = n_k ? n_k[k] : (int)(nk_f[k] + 0.5f);     // packed operand: counts summed as floats (exact)
    const size_t at = (size_t)k * NACT * NF + i;
    apply_weight(W + at, G[at], nk, scale + i % NF, alpha, nk_floor);
}

// The order-pinned multi-rank form (SPEC §5): G and the counts are the sums of the packed operands op(0), op(1), .. op(n - 1), one
// addition at a time in that order (op(r) = where operand r starts).
template <typename Operand>
__device__ __forceinline__ void apply_sum(float *W, Operand op, int n, int n_vf, const float *scale, float alpha, int nk_floor) {
    const int k = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= NACT * NF) return;
    const size_t at = (size_t)k * NACT * NF + i, cnt_at = (size_t)n_vf * NACT * NF + k;
    float g = op(0)[at], nkf = op(0)[cnt_at];
    for (int r = 1; r < n; ++r) {
        g = g + op(r)[at];
        nkf = nkf + op(r)[cnt_at];                               // counts as floats: exact (far below 2^24)
    }
    apply_weight(W + at, g, (int)(nkf + 0.5f), scale + i % NF, alpha, nk_floor);
}

__global__ __launch_bounds__(256) void apply_slots_kernel(float *W, const float *slots, int n_slots, long stride, int n_vf,
                                                          const float *scale, float alpha, int nk_floor) {
    apply_sum(W, [=](int r) { return slots + (size_t)r * stride; }, n_slots, n_vf, scale, alpha, nk_floor);
}

// The peer transport of the order-pinned sum: every rank of a node publishes its packed operand in a region of its
// own (scg_peer_export), reads the others' through IPC mappings and sums all of them in rank order here. Region layout: line 0 the
// epoch word, line 1 the void flags (one per parity), then the two packed operands (parity 0 / 1), each 256-B aligned.
constexpr int PEER_MAX = 8;
constexpr size_t PEER_HDR = 256;               // bytes: epoch line + void line (128 B each)

struct PeerView {
    const float *buf[PEER_MAX][2];             // rank r's packed operand of parity p (own region or IPC mapping)
    const uint32_t *epoch[PEER_MAX];           // rank r's epoch word: the number of exchanges it has published
    const uint32_t *voidw[PEER_MAX];           // rank r's void flags [2], by parity
};

__device__ __forceinline__ bool epoch_reached(uint32_t v, uint32_t need) { return (int32_t)(v - need) >= 0; }   // (wrap-safe)

// Step (a), publish: the void flag of this exchange, a system-scope release, then the epoch. Stream order puts this behind the
// reduce launch that wrote the operand (a kernel boundary: its stores are written back from the XCD's L2 at the launch's end).
__global__ __launch_bounds__(64) void peer_publish_kernel(uint32_t *epoch, uint32_t *voidw, int parity, const int32_t *fail,
                                                          uint32_t value) {
    if (threadIdx.x != 0) return;
    const int32_t f = __hip_atomic_load(fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&voidw[parity], f ? 1u : 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");          // system scope (a peer may sit on another GPU)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // (keep the fence's wait: cdna_hip_programming §6 G16, pitfall 12)
    __hip_atomic_store(epoch, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Step (b), wait: ONE wave, lane r polls rank r's epoch until it reaches `need` (relaxed system-scope loads, s_sleep between
// them), bounded by the 100 MHz wall clock. Then one system-scope acquire and the void flags. The verdict goes to `go` (read by
// apply_peers_kernel, the next launch): 1 = apply, 0 = leave W alone (a peer timed out: SCG_ASYNC_PEER_TIMEOUT; a rank voided
// its step: SCG_ASYNC_STEP_HANDOFF). This is the only kernel that spins.
__global__ __launch_bounds__(64) void peer_wait_kernel(const PeerView P, int n_ranks, int parity, uint32_t need,
                                                       unsigned long long timeout_ticks, int32_t *go, uint32_t *async_word) {
    const int lane = threadIdx.x;
    bool late = false, voided = false;
    if (lane < n_ranks) {
        unsigned long long t0 = 0;
        int spins = 0;
        while (!epoch_reached(__hip_atomic_load(P.epoch[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM), need)) {
            __builtin_amdgcn_s_sleep(2);
            if ((++spins & 63) == 0) {
                const unsigned long long now = __builtin_amdgcn_s_memrealtime();
                if (t0 == 0) t0 = now;
                else if (now - t0 > timeout_ticks) { late = true; break; }
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");          // system scope: the void flags below are the peers' of THIS exchange
    if (lane < n_ranks && !late)
        voided = __hip_atomic_load(&P.voidw[lane][parity], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u;
    const bool any_late = __ballot(late) != 0, any_void = __ballot(voided) != 0;
    if (lane == 0) {
        if (any_late) __hip_atomic_fetch_or(async_word, SCG_ASYNC_PEER_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        else if (any_void) __hip_atomic_fetch_or(async_word, SCG_ASYNC_STEP_HANDOFF, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(go, (any_late || any_void) ? 0 : 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Step (c), apply: apply_slots_kernel's arithmetic on the n_ranks operands of one parity, read through their device pointers.
// It never polls: lane 0 reads the verdict and the peers' epochs, then ONE system-scope acquire (this CU's L1 and its XCD's L2
// may still hold a peer's buffer from exchange e - 2), and the workgroup barrier comes before any operand load.
__global__ __launch_bounds__(256) void apply_peers_kernel(float *W, const PeerView P, int n_ranks, int parity, uint32_t need,
                                                          const int32_t *go, int n_vf, const float *scale, float alpha,
                                                          int nk_floor) {
    __shared__ int s_ok;
    if (threadIdx.x == 0) {
        int ok = __hip_atomic_load(go, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int r = 0; r < n_ranks; ++r)
            ok &= epoch_reached(__hip_atomic_load(P.epoch[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM), need) ? 1 : 0;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
        s_ok = ok;
    }
    __syncthreads();
    if (!s_ok) return;
    apply_sum(W, [&](int r) { return P.buf[r][parity]; }, n_ranks, n_vf, scale, alpha, nk_floor);
}
