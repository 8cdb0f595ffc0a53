// scg_gram_kernel.hpp — SPEC §16.1: gram_kernel, the feature Gram A_g = sum_n phi(s_n) phi(s_n)^T (and b_g = sum_n phi(s_n) yv[n]) of
// segments of recorded states, as an f32 rank-k update on v_mfma_f32_16x16x4_f32 whose operands are built on the fly from the 16-byte
// state: phi is never materialised. Included by scg_kernels.hip for GramArgs and the launch's declaration only; the kernel is compiled
// in scg_gram.hip, a translation unit of its own (what shares a module with the hot kernels changes their code: DESIGN §3.10).
//
// Geometry. The 1296 features are 81 tiles of 16. A wave owns GRAM_R x GRAM_R tiles, a workgroup GRAM_WG x GRAM_WG waves =
// one macro-tile of GRAM_MT tiles a side; the grid is (macro-tiles on or above the diagonal) x (non-empty segments). The last macro-tile
// of a side is short (81 = 13 x 6 + 3): waves past tile 80 only help to build tables. A workgroup walks its segment slab by slab
// (SCG_GRAM_SLAB samples) and a slab in chunks of GRAM_CHUNK samples: all waves build the chunk's AB / CD tables (SPEC §3) into LDS once,
// then every wave, per four samples, turns them into its 2 GRAM_R operand registers — lane (i, k) holds phi_{16 t + i}(sample k) — and
// issues GRAM_R^2 MFMAs into the slab's accumulators P. At the end of a slab the wave adds P to its second set, the segment totals, in
// registers. Nothing is exchanged between workgroups, nothing waits: the kernel raises no asynchronous status and cannot hang.
// The order of every sum is SPEC §16.1's whatever GRAM_R / GRAM_WG / GRAM_CHUNK are: per entry one fma chain over the slab's samples in
// ascending order (the MFMA is that chain over its four k), then the slabs in order.
#pragma once

constexpr int GRAM_SLAB = SCG_GRAM_SLAB;
constexpr int GRAM_MAX_SEG = SCG_GRAM_MAX_SEGMENTS;
#ifndef SCG_GRAM_R
#define SCG_GRAM_R 3                                 // (build parameters of the tiling A/Bs of tools/gram_bench.py)
#endif
#ifndef SCG_GRAM_WG
#define SCG_GRAM_WG 2
#endif
#ifndef SCG_GRAM_WPE
#define SCG_GRAM_WPE 2                               // waves per SIMD the register budget allows for (two workgroups share a CU)
#endif
constexpr int GRAM_R = SCG_GRAM_R;                   // tiles a side per wave: R^2 accumulators of 4 registers, twice (P and the totals)
constexpr int GRAM_WG = SCG_GRAM_WG;                 // waves a side per workgroup (1: every wave builds its own tables)
constexpr int GRAM_TILES = NF / 16;                  // 81
constexpr int GRAM_MT = GRAM_R * GRAM_WG;            // tiles a side per macro-tile: SCG_GRAM_MACRO_TILE features
constexpr int GRAM_ME = (GRAM_TILES + GRAM_MT - 1) / GRAM_MT;
constexpr int GRAM_MACROS = GRAM_ME * (GRAM_ME + 1) / 2;
constexpr int GRAM_THREADS = 64 * GRAM_WG * GRAM_WG;
constexpr int GRAM_CHUNK = 64;                       // samples whose tables the workgroup holds in LDS
constexpr int GRAM_TS = 80;                          // float2 per sample row of the tables (72 used): 160 floats = 32 banks mod 64, so the
                                                     // rows of two neighbouring samples, read at once, start on opposite bank halves
static_assert(NF % 16 == 0 && GRAM_MT * 16 == SCG_GRAM_MACRO_TILE && GRAM_SLAB % GRAM_CHUNK == 0 && GRAM_CHUNK % 4 == 0, "gram geometry");

struct GramArgs {
    const float *x, *y, *vx, *vy, *yv;               // yv and b: both or neither
    float *A, *b;
    int32_t seg[GRAM_MAX_SEG];                       // the non-empty segments: index (A_g = A + seg * 1296^2), first sample, samples
    int64_t start[GRAM_MAX_SEG], count[GRAM_MAX_SEG];
};
// grid = GRAM_MACROS x n_active workgroups of GRAM_THREADS on stream s (defined in scg_gram.hip)
hipError_t launch_feature_gram(const GramArgs &G, int n_active, hipStream_t s);

#ifdef SCG_GRAM_DEFINE_KERNEL
// the table places of feature f (clamped: the tiles of a short macro-tile read a valid place and are never stored): AB at f / 36, CD behind them
__device__ __forceinline__ void gram_places(int f, int &ab, int &cd) {
    f = min(f, NF - 1);
    ab = f / 36; cd = 36 + f % 36;
}
// phi_f of the sample whose table row is `row`, exactly as features_kernel forms it
__device__ __forceinline__ float gram_phi(const float2 *row, int ab_at, int cd_at) {
    const float2 ab = row[ab_at], cd = row[cd_at];
    return fmaf(-ab.y, cd.y, ab.x * cd.x);
}

template <bool RHS>
__global__ __launch_bounds__(GRAM_THREADS, SCG_GRAM_WPE) void gram_kernel(const GramArgs G) {
    __shared__ __attribute__((aligned(16))) float2 s_z1[GRAM_CHUNK][4];
    __shared__ float2 s_tab[GRAM_CHUNK * GRAM_TS];
    __shared__ float s_yv[GRAM_CHUNK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n16 = lane & 15, kk = lane >> 4;                 // MFMA operand lane: row / column n16 of the tile, k index (A, B) or row group (C, D)
    int I = 0, mj = blockIdx.x;                                // macro-tile (I, J), I <= J: the upper triangle row by row
    while (mj >= GRAM_ME - I) { mj -= GRAM_ME - I; ++I; }
    const int J = I + mj;
    const int r0 = GRAM_MT * I + GRAM_R * (wave / GRAM_WG), c0 = GRAM_MT * J + GRAM_R * (wave % GRAM_WG);      // the wave's first row / column tile
    const bool diag = r0 == c0;                                // the block is its own mirror image
    const bool active = c0 < GRAM_TILES && r0 <= c0;           // (a block below the diagonal is the mirror image of one that is computed)
    const bool rhs = RHS && diag;                              // b's rows 16 r0 .. are this wave's
    int ra[GRAM_R], rc[GRAM_R], ca[GRAM_R], cc[GRAM_R];
#pragma unroll
    for (int r = 0; r < GRAM_R; ++r) {
        gram_places(16 * (r0 + r) + n16, ra[r], rc[r]);
        gram_places(16 * (c0 + r) + n16, ca[r], cc[r]);
    }
    const f4v zero4 = (f4v){0.0f, 0.0f, 0.0f, 0.0f};
    f4v tot[GRAM_R][GRAM_R], acc[GRAM_R][GRAM_R], btot[GRAM_R], bacc[GRAM_R];
#pragma unroll
    for (int r = 0; r < GRAM_R; ++r) {
        btot[r] = zero4; bacc[r] = zero4;
#pragma unroll
        for (int c = 0; c < GRAM_R; ++c) { tot[r][c] = zero4; acc[r][c] = zero4; }
    }
    const int64_t first = G.start[blockIdx.y], count = G.count[blockIdx.y];
    for (int64_t s0 = 0; s0 < count; s0 += GRAM_SLAB) {
        const int slab = (int)(count - s0 < (int64_t)GRAM_SLAB ? count - s0 : (int64_t)GRAM_SLAB);
        for (int q0 = 0; q0 < slab; q0 += GRAM_CHUNK) {
            const int m = min(GRAM_CHUNK, slab - q0);          // samples of this chunk; its rows m .. up to the next multiple of 4 are null samples
            const int64_t base = first + s0 + q0;
            __syncthreads();                                   // the tables of the last chunk are consumed
            for (int t = tid; t < GRAM_CHUNK * 4; t += GRAM_THREADS) {
                const int smp = t >> 2, d = t & 3;
                if (smp < m) {
                    const float *src = d == 0 ? G.x : (d == 1 ? G.y : (d == 2 ? G.vx : G.vy));
                    const float v = src[base + smp];
                    s_z1[smp][d] = sincospi_cs(d < 2 ? v : fmaf(v, 0.25f, 0.5f));          // state_powers' Z_d^1
                }
            }
            if (RHS) {
                for (int t = tid; t < GRAM_CHUNK; t += GRAM_THREADS) s_yv[t] = t < m ? G.yv[base + t] : 0.0f;
            }
            __syncthreads();
            for (int t = tid; t < GRAM_CHUNK * 6; t += GRAM_THREADS) {
                const int smp = t % GRAM_CHUNK, cp = t / GRAM_CHUNK;      // cp is wave-uniform
                float2 *row = s_tab + smp * GRAM_TS;
                if (smp < m) {
                    float2 ab[6], cd[6];
                    item_entries(&s_z1[smp][0], cp, ab, cd);
#pragma unroll
                    for (int c = 0; c < 6; ++c) { row[6 * c + cp] = ab[c]; row[36 + 6 * c + cp] = cd[c]; }
                } else if (smp < ((m + 3) & ~3)) {
#pragma unroll
                    for (int c = 0; c < 6; ++c) { row[6 * c + cp] = make_float2(0.0f, 0.0f); row[36 + 6 * c + cp] = make_float2(0.0f, 0.0f); }
                }
            }
            __syncthreads();
            if (active) {
                // per four samples: the operands of the NEXT four are read and formed before this four's products are issued (one wave per
                // SIMD: nothing else hides the LDS round trip); a full chunk's loop is unrolled, a short one runs the same steps
                const float2 *row = s_tab + kk * GRAM_TS;
                float a[GRAM_R], bo[GRAM_R], an[GRAM_R], bn[GRAM_R];
                auto operands = [&](int ks, float (&pa)[GRAM_R], float (&pb)[GRAM_R]) {
#pragma unroll
                    for (int r = 0; r < GRAM_R; ++r) {
                        pa[r] = gram_phi(row + 4 * ks * GRAM_TS, ra[r], rc[r]);
                        pb[r] = gram_phi(row + 4 * ks * GRAM_TS, ca[r], cc[r]);
                    }
                };
                auto step = [&](int ks, bool more) {
                    if (more) operands(ks + 1, an, bn);
#pragma unroll
                    for (int r = 0; r < GRAM_R; ++r) {
#pragma unroll
                        for (int c = 0; c < GRAM_R; ++c) acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], bo[c], acc[r][c], 0, 0, 0);
                    }
                    if (rhs) {                                 // yv as column 0 of a B operand: column 0 of the product is b's chain
                        const float yb = n16 == 0 ? s_yv[4 * ks + kk] : 0.0f;
#pragma unroll
                        for (int r = 0; r < GRAM_R; ++r) bacc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], yb, bacc[r], 0, 0, 0);
                    }
#pragma unroll
                    for (int r = 0; r < GRAM_R; ++r) { a[r] = an[r]; bo[r] = bn[r]; }
                };
                operands(0, a, bo);
                if (m == GRAM_CHUNK) {
#pragma unroll
                    for (int ks = 0; ks < GRAM_CHUNK / 4; ++ks) step(ks, ks + 1 < GRAM_CHUNK / 4);
                } else {
                    const int nks = (m + 3) >> 2;
                    for (int ks = 0; ks < nks; ++ks) step(ks, ks + 1 < nks);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < GRAM_R; ++r) {                     // the slab's P joins the segment's total; the next slab starts from +0
            btot[r] = btot[r] + bacc[r]; bacc[r] = zero4;
#pragma unroll
            for (int c = 0; c < GRAM_R; ++c) { tot[r][c] = tot[r][c] + acc[r][c]; acc[r][c] = zero4; }
        }
    }
    if (!active) return;
    // accumulator lane (n16, kk), register v = entry (row 4 kk + v, column n16) of the tile
    float *Ag = G.A + (size_t)G.seg[blockIdx.y] * NF * NF;
#pragma unroll
    for (int r = 0; r < GRAM_R; ++r) {
        if (r0 + r >= GRAM_TILES) continue;
        const int row = 16 * (r0 + r) + 4 * kk;
#pragma unroll
        for (int c = 0; c < GRAM_R; ++c) {
            if (c0 + c >= GRAM_TILES) continue;
            const int col = 16 * (c0 + c) + n16;
#pragma unroll
            for (int v = 0; v < 4; ++v) Ag[(size_t)(row + v) * NF + col] = tot[r][c][v];
            if (!diag) {                                       // the mirror image (a diagonal block holds its own)
#pragma unroll
                for (int v = 0; v < 4; ++v) Ag[(size_t)col * NF + row + v] = tot[r][c][v];
            }
        }
        if (rhs && n16 == 0) {
#pragma unroll
            for (int v = 0; v < 4; ++v) G.b[(size_t)G.seg[blockIdx.y] * NF + row + v] = btot[r][v];
        }
    }
}
#endif
