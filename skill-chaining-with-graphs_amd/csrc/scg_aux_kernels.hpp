// scg_aux_kernels.hpp — the un-fused kernels: pinball_kernel, features_kernel, predict_kernel and fit_kernel (SPEC §6).
// Included by scg_kernels.hip.
#pragma once

__global__ __launch_bounds__(256) void pinball_kernel(int n, float *x, float *y, float *vx, float *vy,
                                                      const uint8_t *action, float *reward, uint8_t *goal,
                                                      const float *edges, const uint64_t *cellmask, MapScalars ms) {
    // the fused step's physics, wave by wave (pinball_wave_*: free flight in place, (env, edge) pairs on the wave's own lanes)
    __shared__ __attribute__((aligned(16))) float s_edges[MAX_EDGES * 8];
    __shared__ uint32_t s_items[4][PITEMS];
    __shared__ float s_xs[4][4 * 64];
    __shared__ uint8_t s_g[4][64];
    for (int i = threadIdx.x; i < ms.n_edges * 8; i += 256) s_edges[i] = edges[i];
    __syncthreads();
    const int e = blockIdx.x * 256 + threadIdx.x, wv = threadIdx.x >> 6;
    const bool valid = e < n;
    float sx = 0.5f, sy = 0.5f, svx = 0.0f, svy = 0.0f;
    int a = NACT - 1;
    if (valid) { sx = x[e]; sy = y[e]; svx = vx[e]; svy = vy[e]; a = action[e]; }
    bool g, par;
    const int groups = pinball_wave_prepare_any(s_edges, cellmask, ms, valid, sx, sy, svx, svy, a, g, par, s_items[wv], s_xs[wv], 64);
    wave_lds_sync();
    for (int q = 0; q < groups; ++q) pinball_wave_group(s_edges, ms, s_items[wv] + 64 * q, s_xs[wv], 64, s_g[wv]);
    wave_lds_sync();
    const float r = pinball_wave_finish(par, sx, sy, svx, svy, a, g, s_xs[wv], 64, s_g[wv]);
    if (valid) {
        x[e] = sx; y[e] = sy; vx[e] = svx; vy[e] = svy;
        reward[e] = r; goal[e] = g ? 1 : 0;
    }
}

// one wavefront per env: materialises phi[n][1296] (the fused path never does this)
__global__ __launch_bounds__(64) void features_kernel(int n, const float *x, const float *y, const float *vx,
                                                      const float *vy, float *phi) {
    __shared__ float2 s_pw[20];
    __shared__ float2 s_abcd[72];
    const int lane = threadIdx.x;
    for (int e = blockIdx.x; e < n; e += gridDim.x) {
        if (lane == 0) state_powers(x[e], y[e], vx[e], vy[e], s_pw);
        wave_lds_sync();
        for (int p = lane; p < 72; p += 64) {
            const int q = p % 36, d0 = p < 36 ? 0 : 2;
            float2 v = pow_at(s_pw, d0 + 1, q % 6);                       // row 0; row c = row c - 1 times Z_d0^1
            for (int c = 1; c <= q / 6; ++c) v = cmul(v, pow_at(s_pw, d0, 1));
            s_abcd[p] = v;
        }
        wave_lds_sync();
        for (int f = lane; f < NF; f += 64) {
            const float2 ab = s_abcd[f / 36], cd = s_abcd[36 + f % 36];
            phi[(size_t)e * NF + f] = fmaf(-ab.y, cd.y, ab.x * cd.x);
        }
        wave_lds_sync();
    }
}

__global__ __launch_bounds__(256) void predict_kernel(int n, const float *x, const float *y, const float *w8,
                                                      uint8_t *out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < n) out[e] = clf_z(w8, x[e], y[e]) > 0.0f ? 1 : 0;
}

// SPEC §6: FIT_G workgroups of FIT_T threads per option. Thread gamma = j FIT_T + tau owns examples i = gamma (mod
// FIT_G FIT_T) and keeps the first FIT_EPT of them in registers for all iterations (65 536 examples per option; more are
// re-read from memory). Per iteration: per-thread fma chains -> butterfly inside each wave -> the workgroup's 16 waves in
// order -> the option's FIT_G workgroup partials in order, exchanged through global memory behind a counter barrier
// (the partials are double-buffered by iteration parity; FIT_G x n_fit <= 64 workgroups are co-resident by construction,
// and every spin is bounded). One 256-thread workgroup per option took 12.6 ms for 40 000 examples x 400 iterations.
constexpr int FIT_G = 8, FIT_T = 1024, FIT_EPT = 8, FIT_BATCH = 8;
constexpr int FIT_STRIDE = FIT_G * FIT_T;

__global__ __launch_bounds__(FIT_T) void fit_kernel(const float *xy, const uint8_t *label, const int32_t *offsets,
                                                    float *w, int iters, float lr, float l2, int q0,
                                                    unsigned long long *part, unsigned long long timeout_ticks,
                                                    uint32_t *async_word) {
    __shared__ float sw[8];
    __shared__ float swave[FIT_T / 64][6];
    __shared__ int s_abort;
    const int ql = blockIdx.y, q = q0 + ql, j = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = offsets[q], M = offsets[q + 1] - offsets[q];
    if (M <= 0) return;                                   // the option's FIT_G workgroups all take this exit
    if (tid < 8) sw[tid] = w[CLF_STRIDE * q + tid];
    if (tid == 0) s_abort = 0;
    const int gamma = j * FIT_T + tid;
    float cu[FIT_EPT], cv[FIT_EPT], cl[FIT_EPT];
#pragma unroll
    for (int e = 0; e < FIT_EPT; ++e) {
        const int i = gamma + FIT_STRIDE * e;
        cu[e] = 0.0f; cv[e] = 0.0f; cl[e] = 0.0f;
        if (i < M) {
            cu[e] = fmaf(xy[2 * (size_t)(i0 + i)], 2.0f, -1.0f);
            cv[e] = fmaf(xy[2 * (size_t)(i0 + i) + 1], 2.0f, -1.0f);
            cl[e] = (float)label[i0 + i];
        }
    }
    const float invM = 1.0f / (float)M;
    unsigned long long *my_part = part + (size_t)ql * 2 * FIT_G * 8;
    for (int it = 0; it < iters; ++it) {
        __syncthreads();
        float wl[6];
#pragma unroll
        for (int jj = 0; jj < 6; ++jj) wl[jj] = sw[jj];
        float g[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        auto one = [&](float u, float v, float lbl) {
            const float psi[6] = {1.0f, u, v, u * u, u * v, v * v};
            float z = wl[0];
            z = fmaf(wl[1], u, z); z = fmaf(wl[2], v, z);
            z = fmaf(wl[3], psi[3], z); z = fmaf(wl[4], psi[4], z); z = fmaf(wl[5], psi[5], z);
            const float e = sigmoid_spec(z) - lbl;
#pragma unroll
            for (int jj = 0; jj < 6; ++jj) g[jj] = fmaf(e, psi[jj], g[jj]);
        };
#pragma unroll
        for (int e = 0; e < FIT_EPT; ++e)
            if (gamma + FIT_STRIDE * e < M) one(cu[e], cv[e], cl[e]);
        for (int i = gamma + FIT_STRIDE * FIT_EPT; i < M; i += FIT_STRIDE)          // beyond the register-resident part
            one(fmaf(xy[2 * (size_t)(i0 + i)], 2.0f, -1.0f), fmaf(xy[2 * (size_t)(i0 + i) + 1], 2.0f, -1.0f), (float)label[i0 + i]);
#pragma unroll
        for (int jj = 0; jj < 6; ++jj) {
            g[jj] = wave_sum(g[jj]);
            if (lane == 0) swave[wave][jj] = g[jj];
        }
        __syncthreads();
        // exchange of the workgroup partials: every value travels as ONE 64-bit word {iteration tag, float bits}, stored
        // and polled with 64-bit relaxed agent-scope atomics — a value that carries the awaited tag is valid by itself, so
        // the exchange costs one store and one (polled) load round trip; buffers alternate by iteration parity (a fast
        // workgroup writes iteration it + 1 while a slow one still reads iteration it)
        unsigned long long *buf = my_part + (it & 1) * FIT_G * 8;
        const unsigned long long tag = (unsigned long long)(unsigned)(it + 1) << 32;
        if (tid < 6) {
            float ps = swave[0][tid];
#pragma unroll
            for (int wv = 1; wv < FIT_T / 64; ++wv) ps = ps + swave[wv][tid];
            __hip_atomic_store(&buf[j * 8 + tid], tag | __float_as_uint(ps), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (wave == 0) {
            unsigned long long v = tag;
            if (lane < 6 * FIT_G) {                          // lane -> (workgroup lane / 6, component lane % 6)
                const unsigned long long *src = &buf[(lane / 6) * 8 + lane % 6];
                // The option's FIT_G workgroups must all be running for this to complete. A plain launch (and a
                // cooperative one: MI355X_MICROARCH.md, residency) promises that only on an otherwise idle card: another
                // stream or process may hold CUs. A late partner is waited for on the 100 MHz wall clock — seconds,
                // not a spin count — and a partner that never shows up ABORTS the fit: weights left as they were,
                // SCG_ASYNC_FIT_TIMEOUT raised in the ctx's host-visible status word (scg_async_status) by the
                // problem's workgroup 0, the only one that writes the row.
                unsigned long long t0 = 0;
                int spins = 0;
                while (((v = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) >> 32) != (tag >> 32)) {
                    __builtin_amdgcn_s_sleep(1);
                    if ((++spins & 255) == 0) {
                        const unsigned long long now = __builtin_amdgcn_s_memrealtime();
                        if (t0 == 0) t0 = now;
                        else if (now - t0 > timeout_ticks) { s_abort = 1; break; }
                    }
                }
            }
            const float val = __uint_as_float((unsigned)v);
            const int c = lane < 6 ? lane : 0;
            float gs = __shfl(val, c, 64);                   // the FIT_G group sums in order
#pragma unroll
            for (int jw = 1; jw < FIT_G; ++jw) gs = gs + __shfl(val, jw * 6 + c, 64);
            if (lane < 6) {
                const float reg = (lane > 0) ? l2 * sw[lane] : 0.0f;
                sw[lane] = sw[lane] - lr * ((gs * invM) + reg);
            }
        }
        __syncthreads();
        if (s_abort) break;
    }
    __syncthreads();
    if (s_abort) {                                        // no silent NaN row: w keeps its old value, the host is told.
        // Workgroup 0 of the problem alone decides: it is the one that writes the row, so "status bit raised" and "row left
        // untouched" are the same event. A partner that gives up merely exits (workgroup 0 then either holds everything it
        // needs — the partner had published its last partial — and finishes exactly, or runs out of patience itself).
        if (j == 0 && tid == 0 && async_word)
            __hip_atomic_fetch_or(async_word, SCG_ASYNC_FIT_TIMEOUT | (0x100u << (q & 15)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    if (j == 0 && tid < 6) w[CLF_STRIDE * q + tid] = sw[tid];
}
