// scg_basis_kernels.hpp — SPEC §18's two small kernels, templated on GramOrder<p> (scg_gram_kernel.hpp) and instantiated in scg_basis.hip
// only, and the launches scg_kernels.hip calls. Both are plain vector-pipe kernels, one wavefront a workgroup: reporting, not the hot path.
//   basis_features_kernel   phi[n][F] of order p, features_kernel's operations in features_kernel's order (at order 5 its bits; the entry
//                           point launches features_kernel itself there)
//   basis_values_kernel     out[r][n] = sum_f V[r][f] phi_f(s_n) for r < m <= 8 in §18.3's order: per c12 an fma chain T over c34 from +0,
//                           the T added in c12 order from +0. phi is formed in registers, never stored.
//   logistic_terms_kernel   SPEC §23.1: p = sigmoid_spec(z), e = l - p, rw = sqrt(p (1 - p)) per sample, every step one binary32 operation
//   classifier_logits_kernel  SPEC §24.2: z = clf_z(w8, x, y) per point, the value whose sign predict_kernel (scg_aux_kernels.hpp) tests
#pragma once

// grid-stride launches on stream s (scg_basis.hip); st = {x, y, vx, vy}. The Gram launches read G.s[0] only.
hipError_t launch_basis_gram_3(const GramArgs &G, int n_active, hipStream_t s);
hipError_t launch_basis_gram_7(const GramArgs &G, int n_active, hipStream_t s);
hipError_t launch_basis_features(int order, int64_t n, const float *const *st, float *phi, hipStream_t s);      // order 3 or 7
hipError_t launch_basis_values(int order, int64_t n, const float *const *st, const float *V, int m, float *out, hipStream_t s);
hipError_t launch_basis_gram_irls_3(const GramArgs &G, int n_active, hipStream_t s);      // SPEC §23.2: G.rw, G.yv = e, G.b = grad
hipError_t launch_basis_gram_irls_7(const GramArgs &G, int n_active, hipStream_t s);
hipError_t launch_logistic_terms(int64_t n, const float *z, const uint8_t *label, float *p, float *rw, float *e, hipStream_t s);
hipError_t launch_classifier_logits(int n, const float *x, const float *y, const float *w8, float *z, hipStream_t s);      // n >= 1

constexpr int BASIS_VALUES_SAMPLES = 8;              // samples a wavefront of basis_values_kernel takes at once: a weight is loaded once for all of them

// Z_d^1 of state variable d (state_powers' first step)
__device__ __forceinline__ float2 basis_z1(const float *x, const float *y, const float *vx, const float *vy, int64_t e, int d) {
    const float v = (d == 0 ? x : (d == 1 ? y : (d == 2 ? vx : vy)))[e];
    return sincospi_cs(d < 2 ? v : fmaf(v, 0.25f, 0.5f));
}
// entry q of a sample's 2 P2 table entries (AB, then CD) from its four Z_d^1: row 0 is the power chain, row c = row c - 1 times Z_d0^1
template <class O>
__device__ __forceinline__ float2 basis_entry(const float2 *z1, int q) {
    const int e = q % O::P2, d0 = q < O::P2 ? 0 : 2;
    const float2 zr = z1[d0];
    float2 v = zpow_sel<O::P1>(z1[d0 + 1], e % O::P1);
    for (int c = 1; c <= e / O::P1; ++c) v = cmul(v, zr);
    return v;
}

template <class O>
__global__ __launch_bounds__(64) void basis_features_kernel(int64_t n, const float *x, const float *y, const float *vx, const float *vy,
                                                            float *phi) {
    constexpr int P2 = O::P2, F = O::F;
    __shared__ float2 s_z1[4];
    __shared__ float2 s_abcd[2 * P2];
    const int lane = threadIdx.x;
    for (int64_t e = blockIdx.x; e < n; e += gridDim.x) {
        if (lane < 4) s_z1[lane] = basis_z1(x, y, vx, vy, e, lane);
        wave_lds_sync();
        for (int q = lane; q < 2 * P2; q += 64) s_abcd[q] = basis_entry<O>(s_z1, q);
        wave_lds_sync();
        for (int f = lane; f < F; f += 64) {
            const float2 ab = s_abcd[f / P2], cd = s_abcd[P2 + f % P2];
            phi[(size_t)e * F + f] = fmaf(-ab.y, cd.y, ab.x * cd.x);
        }
        wave_lds_sync();
    }
}

template <class O>
__global__ __launch_bounds__(64) void basis_values_kernel(int64_t n, const float *x, const float *y, const float *vx, const float *vy,
                                                          const float *V, int m, float *out) {
    constexpr int SB = BASIS_VALUES_SAMPLES, P2 = O::P2, F = O::F;
    static_assert(P2 <= 64 && 4 * SB <= 64, "lane = c12");
    __shared__ float2 s_z1[SB][4];
    __shared__ float2 s_ab[SB][P2], s_cd[SB][P2];
    __shared__ float s_t[SB][P2];
    const int lane = threadIdx.x;
    const int64_t groups = (n + SB - 1) / SB;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t e0 = g * SB;
        const int cnt = (int)(n - e0 < (int64_t)SB ? n - e0 : (int64_t)SB);
        if (lane < 4 * SB)                                     // (a group's missing samples: any finite state, never stored)
            s_z1[lane >> 2][lane & 3] = (lane >> 2) < cnt ? basis_z1(x, y, vx, vy, e0 + (lane >> 2), lane & 3) : make_float2(1.0f, 0.0f);
        wave_lds_sync();
        for (int t = lane; t < SB * 2 * P2; t += 64) {
            const int s = t / (2 * P2), q = t % (2 * P2);
            const float2 v = basis_entry<O>(s_z1[s], q);
            if (q < P2) s_ab[s][q] = v; else s_cd[s][q - P2] = v;
        }
        wave_lds_sync();
        float2 ab[SB];                                         // lane = c12
#pragma unroll
        for (int s = 0; s < SB; ++s) ab[s] = s_ab[s][lane < P2 ? lane : 0];
        for (int r = 0; r < m; ++r) {
            if (lane < P2) {
                float T[SB];
#pragma unroll
                for (int s = 0; s < SB; ++s) T[s] = 0.0f;
                const float *Vr = V + (size_t)r * F + lane * P2;
                for (int c34 = 0; c34 < P2; ++c34) {
                    const float w = Vr[c34];
#pragma unroll
                    for (int s = 0; s < SB; ++s) {
                        const float2 cd = s_cd[s][c34];
                        T[s] = fmaf(w, fmaf(-ab[s].y, cd.y, ab[s].x * cd.x), T[s]);
                    }
                }
#pragma unroll
                for (int s = 0; s < SB; ++s) s_t[s][lane] = T[s];
            }
            wave_lds_sync();
            if (lane < cnt) {
                float o = 0.0f;
                for (int c12 = 0; c12 < P2; ++c12) o = o + s_t[lane][c12];
                out[(size_t)r * n + e0 + lane] = o;
            }
            wave_lds_sync();
        }
    }
}

// SPEC §23.1. The build has -ffp-contract=off, so 1 - p and p q stay one subtraction and one multiply; sqrtf is the correctly rounded
// binary32 root (no fast-math anywhere in this library). p (1 - p) is +0 or normal: p >= 0x1.666d0ep-126, and 1 - p >= 2^-24 unless p = 1.
// (A template as the two above, so that scg_basis.hip alone holds its code.)
constexpr int LOGISTIC_THREADS = 256;
template <int THREADS>
__global__ __launch_bounds__(THREADS) void logistic_terms_kernel(int64_t n, const float *z, const uint8_t *label, float *p, float *rw,
                                                                 float *e) {
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
        const float pv = sigmoid_spec(z[i]);
        const float l = label[i] != 0 ? 1.0f : 0.0f;
        const float q = 1.0f - pv;
        const float sv = pv * q;
        p[i] = pv;
        rw[i] = sqrtf(sv);
        e[i] = l - pv;
    }
}

// SPEC §24.2: predict_kernel's launch shape and its one call of clf_z (SPEC §4.1's chain), stored before the comparison. (A template as
// the one above, so that scg_basis.hip alone holds its code.)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void classifier_logits_kernel(int n, const float *x, const float *y, const float *w8, float *z) {
    const int e = blockIdx.x * THREADS + threadIdx.x;
    if (e < n) z[e] = clf_z(w8, x[e], y[e]);
}
