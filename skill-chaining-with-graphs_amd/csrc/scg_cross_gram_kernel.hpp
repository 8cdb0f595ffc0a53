// scg_cross_gram_kernel.hpp — SPEC §17.1: cross_gram_kernel, the cross-feature Gram C_g = sum_n phi(s_n) phi(s2_n)^T between a recorded
// state and its successor, per segment, on v_mfma_f32_16x16x4_f32 with both operands built on the fly from the two 16-byte states.
// Included by scg_kernels.hip for CrossGramArgs and the launch's declaration only; the kernel is compiled in scg_cross_gram.hip, a
// translation unit of its own (what shares a module with the hot kernels changes their code: DESIGN §3.10).
//
// Geometry: gram_kernel's (scg_gram_kernel.hpp), with what the missing symmetry changes. A wave owns CGRAM_R x CGRAM_R
// tiles of 16, a workgroup CGRAM_WG x CGRAM_WG waves = one macro-tile of SCG_CROSS_GRAM_MACRO_TILE features a side, and EVERY macro-tile
// of the square is computed: no mirror store, no diagonal case. The grid is (macro-tiles) x (non-empty segments); the host lists the
// segments longest first, so the long chains start first. A chunk of CGRAM_CHUNK samples holds TWO table sets in LDS, one of s (the row
// operands read only this one) and one of s2 (the column operands); both are built whole. Per entry the order is SPEC §17.1's whatever
// the geometry: one fma chain over the slab's samples in ascending order (the MFMA is that chain over its four k), then the slabs in
// order. Nothing is exchanged between workgroups and nothing waits: no asynchronous status, no hang.
#pragma once

#ifndef SCG_CROSS_GRAM_R
#define SCG_CROSS_GRAM_R 3
#endif
#ifndef SCG_CROSS_GRAM_WG
#define SCG_CROSS_GRAM_WG 2
#endif
#ifndef SCG_CROSS_GRAM_CHUNK
#define SCG_CROSS_GRAM_CHUNK 32                      // two table sets of 32 samples: 43 008 B of LDS, two workgroups a CU as the registers allow
#endif
#ifndef SCG_CROSS_GRAM_CP_FAST
#define SCG_CROSS_GRAM_CP_FAST 1                     // how the table build is dealt to the lanes; 0 is gram_kernel's deal, whose writes all
                                                     // meet on one LDS bank (rows are 160 floats apart): 1.5 - 1.7 x slower
#endif
constexpr int CGRAM_R = SCG_CROSS_GRAM_R;           // tiles a side per wave: R^2 accumulators of 4 registers, twice (the slab's and the totals)
constexpr int CGRAM_WG = SCG_CROSS_GRAM_WG;          // waves a side per workgroup
constexpr int CGRAM_TILES = NF / 16;                 // 81
constexpr int CGRAM_MT = CGRAM_R * CGRAM_WG;         // tiles a side per macro-tile
constexpr int CGRAM_ME = (CGRAM_TILES + CGRAM_MT - 1) / CGRAM_MT;
constexpr int CGRAM_MACROS = CGRAM_ME * CGRAM_ME;    // the whole square
constexpr int CGRAM_THREADS = 64 * CGRAM_WG * CGRAM_WG;
constexpr int CGRAM_CHUNK = SCG_CROSS_GRAM_CHUNK;    // samples whose two table sets the workgroup holds in LDS
constexpr int CGRAM_TS = 80;                         // float2 per sample row of a table (72 used): gram_kernel's GRAM_TS, for its reason
static_assert(NF % 16 == 0 && CGRAM_MT * 16 == SCG_CROSS_GRAM_MACRO_TILE && SCG_GRAM_SLAB % CGRAM_CHUNK == 0 && CGRAM_CHUNK % 4 == 0,
              "cross gram geometry");

struct CrossGramArgs {
    const float *s[2][4];                            // x, y, vx, vy of s and of s2 (they may alias)
    float *C;
    int32_t seg[SCG_GRAM_MAX_SEGMENTS];              // the non-empty segments, longest first: index (C_g = C + seg * 1296^2), first sample, samples
    int64_t start[SCG_GRAM_MAX_SEGMENTS], count[SCG_GRAM_MAX_SEGMENTS];
};
// grid = CGRAM_MACROS x n_active workgroups of CGRAM_THREADS on stream s (defined in scg_cross_gram.hip)
hipError_t launch_feature_cross_gram(const CrossGramArgs &G, int n_active, hipStream_t s);

#ifdef SCG_CROSS_GRAM_DEFINE_KERNEL
__global__ __launch_bounds__(CGRAM_THREADS, 2) void cross_gram_kernel(const CrossGramArgs G) {
    __shared__ __attribute__((aligned(16))) float2 s_z1[2][CGRAM_CHUNK][4];
    __shared__ float2 s_tab[2][CGRAM_CHUNK * CGRAM_TS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n16 = lane & 15, kk = lane >> 4;                 // MFMA operand lane: row / column n16 of the tile, k index (A, B) or row group (C, D)
    const int I = blockIdx.x / CGRAM_ME, J = blockIdx.x % CGRAM_ME;
    const int r0 = CGRAM_MT * I + CGRAM_R * (wave / CGRAM_WG), c0 = CGRAM_MT * J + CGRAM_R * (wave % CGRAM_WG);    // the wave's first row / column tile
    const bool active = r0 < CGRAM_TILES && c0 < CGRAM_TILES;  // (the last macro-tile of a side is short: its other waves only help to build)
    int ra[CGRAM_R], rc[CGRAM_R], ca[CGRAM_R], cc[CGRAM_R];
#pragma unroll
    for (int r = 0; r < CGRAM_R; ++r) {
        gram_places(16 * (r0 + r) + n16, ra[r], rc[r]);
        gram_places(16 * (c0 + r) + n16, ca[r], cc[r]);
    }
    const f4v zero4 = (f4v){0.0f, 0.0f, 0.0f, 0.0f};
    f4v tot[CGRAM_R][CGRAM_R], acc[CGRAM_R][CGRAM_R];
#pragma unroll
    for (int r = 0; r < CGRAM_R; ++r) {
#pragma unroll
        for (int c = 0; c < CGRAM_R; ++c) { tot[r][c] = zero4; acc[r][c] = zero4; }
    }
    const int64_t first = G.start[blockIdx.y], count = G.count[blockIdx.y];
    for (int64_t s0 = 0; s0 < count; s0 += SCG_GRAM_SLAB) {
        const int slab = (int)(count - s0 < (int64_t)SCG_GRAM_SLAB ? count - s0 : (int64_t)SCG_GRAM_SLAB);
        for (int q0 = 0; q0 < slab; q0 += CGRAM_CHUNK) {
            const int m = min(CGRAM_CHUNK, slab - q0);         // samples of this chunk; its rows m .. up to the next multiple of 4 are null samples
            const int64_t base = first + s0 + q0;
            __syncthreads();                                   // the tables of the last chunk are consumed
            for (int t = tid; t < 2 * CGRAM_CHUNK * 4; t += CGRAM_THREADS) {
                const int set = t / (CGRAM_CHUNK * 4), smp = (t >> 2) % CGRAM_CHUNK, d = t & 3;
                if (smp < m) {
                    const float v = G.s[set][d][base + smp];
                    s_z1[set][smp][d] = sincospi_cs(d < 2 ? v : fmaf(v, 0.25f, 0.5f));     // state_powers' Z_d^1
                }
            }
            __syncthreads();
            for (int t = tid; t < 2 * CGRAM_CHUNK * 6; t += CGRAM_THREADS) {
                const int set = t / (CGRAM_CHUNK * 6), u = t % (CGRAM_CHUNK * 6);
#if SCG_CROSS_GRAM_CP_FAST
                const int smp = u / 6, cp = u % 6;                        // neighbouring lanes write neighbouring entries of one row
#else
                const int smp = u % CGRAM_CHUNK, cp = u / CGRAM_CHUNK;    // gram_kernel's deal: neighbouring lanes write one entry of neighbouring rows
#endif
                float2 *row = s_tab[set] + smp * CGRAM_TS;
                if (smp < m) {
                    float2 ab[6], cd[6];
                    item_entries(&s_z1[set][smp][0], cp, ab, cd);
#pragma unroll
                    for (int c = 0; c < 6; ++c) { row[6 * c + cp] = ab[c]; row[36 + 6 * c + cp] = cd[c]; }
                } else if (smp < ((m + 3) & ~3)) {
#pragma unroll
                    for (int c = 0; c < 6; ++c) { row[6 * c + cp] = make_float2(0.0f, 0.0f); row[36 + 6 * c + cp] = make_float2(0.0f, 0.0f); }
                }
            }
            __syncthreads();
            if (active) {
                // per four samples, as in gram_kernel: the operands of the NEXT four are read and formed before this four's products are
                // issued; a full chunk's loop is unrolled, a short one runs the same steps
                const float2 *rowa = s_tab[0] + kk * CGRAM_TS, *rowb = s_tab[1] + kk * CGRAM_TS;
                float a[CGRAM_R], bo[CGRAM_R], an[CGRAM_R], bn[CGRAM_R];
                auto operands = [&](int ks, float (&pa)[CGRAM_R], float (&pb)[CGRAM_R]) {
#pragma unroll
                    for (int r = 0; r < CGRAM_R; ++r) {
                        pa[r] = gram_phi(rowa + 4 * ks * CGRAM_TS, ra[r], rc[r]);
                        pb[r] = gram_phi(rowb + 4 * ks * CGRAM_TS, ca[r], cc[r]);
                    }
                };
                auto step = [&](int ks, bool more) {
                    if (more) operands(ks + 1, an, bn);
#pragma unroll
                    for (int r = 0; r < CGRAM_R; ++r) {
#pragma unroll
                        for (int c = 0; c < CGRAM_R; ++c) acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], bo[c], acc[r][c], 0, 0, 0);
                    }
#pragma unroll
                    for (int r = 0; r < CGRAM_R; ++r) { a[r] = an[r]; bo[r] = bn[r]; }
                };
                operands(0, a, bo);
                if (m == CGRAM_CHUNK) {
#pragma unroll
                    for (int ks = 0; ks < CGRAM_CHUNK / 4; ++ks) step(ks, ks + 1 < CGRAM_CHUNK / 4);
                } else {
                    const int nks = (m + 3) >> 2;
                    for (int ks = 0; ks < nks; ++ks) step(ks, ks + 1 < nks);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < CGRAM_R; ++r) {                    // the slab's sums join the segment's totals; the next slab starts from +0
#pragma unroll
            for (int c = 0; c < CGRAM_R; ++c) { tot[r][c] = tot[r][c] + acc[r][c]; acc[r][c] = zero4; }
        }
    }
    if (!active) return;
    // accumulator lane (n16, kk), register v = entry (row 4 kk + v, column n16) of the tile
    float *Cg = G.C + (size_t)G.seg[blockIdx.y] * NF * NF;
#pragma unroll
    for (int r = 0; r < CGRAM_R; ++r) {
        if (r0 + r >= CGRAM_TILES) continue;
        const int row = 16 * (r0 + r) + 4 * kk;
#pragma unroll
        for (int c = 0; c < CGRAM_R; ++c) {
            if (c0 + c >= CGRAM_TILES) continue;
            const int col = 16 * (c0 + c) + n16;
#pragma unroll
            for (int v = 0; v < 4; ++v) Cg[(size_t)(row + v) * NF + col] = tot[r][c][v];
        }
    }
}
#endif
