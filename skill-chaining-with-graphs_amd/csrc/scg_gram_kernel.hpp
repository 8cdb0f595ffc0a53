// scg_gram_kernel.hpp — SPEC §16.1, §17.1 and §18: gram_kernel, the feature Gram of segments of recorded states as an f32 rank-k update on
// v_mfma_f32_16x16x4_f32 whose operands are built on the fly from the 16-byte state: phi is never materialised. One template, two shapes:
//   symmetric (GramSym)   A_g = sum_n phi(s_n) phi(s_n)^T, and with RHS b_g = sum_n phi(s_n) yv[n]: the macro-tiles on or above the
//                         diagonal are computed and every block is stored with its mirror image; one table set of 64 samples in LDS;
//                         or, SPEC §20.1, B_g[c] = sum_n phi(s_n) Y[c][n] for up to 16 targets c: the columns of the MFMA that forms b;
//                         or, SPEC §22.1 (WEIGHTED), A and that B with a root weight per sample on every operand: sum_n rw_n^2 phi phi^T
//                         or, SPEC §23.2 (IRLS), that weighted A as the Hessian H and, beside it, the UNWEIGHTED b for yv = e as grad
//   cross (GramCross)     C_g = sum_n phi(s_n) phi(s2_n)^T between a state and its successor: every macro-tile of the square, no mirror
//                         store, no diagonal case; TWO table sets of 32 samples, s's for the row operands and s2's for the column operands
// and, for the symmetric shape, the basis order p of SPEC §18 (GramBasis<p>: 3 or 7 next to GramSym's 5; GramOrder<p> holds what follows
// from p). The order-5 shapes are instantiated in scg_gram.hip only, a translation unit of its own (what shares a module with the hot
// kernels changes their code: DESIGN §3.10), the other orders in scg_basis.hip; scg_kernels.hip includes this header for
// GramArgs and the launches' declarations and instantiates nothing.
//
// Geometry. The F features are F / 16 tiles of 16 (order 5: 81). A wave owns R x R tiles, a workgroup
// WG x WG waves = one macro-tile of MT tiles a side; the grid is (macro-tiles) x (non-empty segments). The last macro-tile of a side
// is short (81 = 13 x 6 + 3; 16 = 2 x 6 + 4; 256 = 42 x 6 + 4): waves past the last tile only help to build tables. A workgroup walks
// its segment slab by slab (SCG_GRAM_SLAB samples) and
// a slab in chunks of CHUNK samples: all waves build the chunk's AB / CD tables (SPEC §3) into LDS once, then every wave, per four
// samples, turns them into its 2 R operand registers — lane (i, k) holds phi_{16 t + i}(sample k) — and issues R^2 MFMAs into the slab's
// accumulators P. At the end of a slab the wave adds P to its second set, the segment totals, in registers. Nothing is exchanged
// between workgroups, nothing waits: the kernel raises no asynchronous status and cannot hang.
// The order of every sum is SPEC §16.1's whatever R / WG / CHUNK are: per entry one fma chain over the slab's samples in ascending order
// (the MFMA is that chain over its four k), then the slabs in order.
#pragma once

#ifndef SCG_GRAM_R
#define SCG_GRAM_R 3                                 // (build parameters of the tiling A/Bs of tools/gram_bench.py)
#endif
#ifndef SCG_GRAM_WG
#define SCG_GRAM_WG 2
#endif
#ifndef SCG_GRAM_WPE
#define SCG_GRAM_WPE 2                               // waves per SIMD the register budget allows for (two workgroups share a CU)
#endif
#ifndef SCG_CROSS_GRAM_R
#define SCG_CROSS_GRAM_R 3                           // (build parameters of the A/Bs of tools/cross_gram_bench.py)
#endif
#ifndef SCG_CROSS_GRAM_WG
#define SCG_CROSS_GRAM_WG 2
#endif
#ifndef SCG_CROSS_GRAM_CHUNK
#define SCG_CROSS_GRAM_CHUNK 32                      // two table sets of 32 samples: 43 008 B of LDS, two workgroups a CU as the registers allow
#endif
#ifndef SCG_CROSS_GRAM_CP_FAST
#define SCG_CROSS_GRAM_CP_FAST 1                     // how the table build is dealt to the lanes (GramShape::FAST_DEAL)
#endif
#ifndef SCG_BASIS_GRAM_CHUNK
#define SCG_BASIS_GRAM_CHUNK 64                      // (build parameter of tools/gram_bench.py --order: the chunk of the orders 3 and 7)
#endif

constexpr int GRAM_SLAB = SCG_GRAM_SLAB;
constexpr int GRAM_MAX_SEG = SCG_GRAM_MAX_SEGMENTS;
constexpr int GRAM_TILES = NF / 16;                  // 81
constexpr int GRAM_TS = 80;                          // float2 per sample row of a table (72 used): 160 floats = 32 banks mod 64, so the
                                                     // rows of two neighbouring samples, read at once, start on opposite bank halves
static_assert(NF % 16 == 0, "gram geometry");

// what follows from the basis order p (SPEC §18): P1 = p + 1 entries a table row, P2 = P1^2 AB (and CD) entries a sample, F = P2^2
// features; the table row of a sample — 2 P2 float2 used of TS, TS = 16 mod 32 float2 at every order, so that the rows of two
// neighbouring samples start on opposite halves of the 64 banks a ds_read_b64 sees —; and the row's swizzle. A power
// of two P1 makes a row's length a multiple of the 32 banks a ds_write_b64 sees, and the lanes of a 16-lane write group, (sample,
// entry column) = (lane / P1, lane mod P1), would meet 16 / P1 deep on 2 P1 banks: the sample with index s (mod 16 / P1) keeps its
// entry e at e ^ (P1 s) instead — its rows of P1 entries permuted —, which spreads a group over all 32 banks. A reader lane always
// reads the samples 4 ks + kk, so its s is a constant it folds into its places once. Order 5 (P1 = 6) has no such swizzle.
template <int ORDER_>
struct GramOrder {
    static_assert(ORDER_ == 3 || ORDER_ == 5 || ORDER_ == 7, "SPEC §18's orders");
    static constexpr int ORDER = ORDER_, P1 = ORDER_ + 1, P2 = P1 * P1, F = P2 * P2, TILES = F / 16;
    static constexpr int TS = ORDER_ == 5 ? GRAM_TS : 2 * P2 + 16;
    static constexpr int SWZ_MASK = ORDER_ == 5 ? 0 : 16 / P1 - 1;
    static_assert(F % 16 == 0 && TS % 32 == 16 && TS >= 2 * P2, "gram geometry");
};
static_assert(GramOrder<5>::F == NF && GramOrder<5>::TILES == GRAM_TILES && GramOrder<5>::P2 == 36, "order 5 is SPEC §3");

// everything the shapes differ in
template <bool CROSS_, int R_, int WG_, int WPE_, int CHUNK_, bool FAST_DEAL_, int ORDER_ = 5>
struct GramShape : GramOrder<ORDER_> {
    using O = GramOrder<ORDER_>;
    static constexpr bool CROSS = CROSS_;            // the whole square from two table sets, or the upper triangle and its mirror from one
    static constexpr int R = R_;                     // tiles a side per wave: R^2 accumulators of 4 registers, twice (P and the totals)
    static constexpr int WG = WG_;                   // waves a side per workgroup (1: every wave builds its own tables)
    static constexpr int WPE = WPE_;                 // waves per SIMD of the launch bounds
    static constexpr int CHUNK = CHUNK_;             // samples whose tables the workgroup holds in LDS
    // the table build's deal: (entry column = lane mod P1, sample = lane / P1), or (sample = lane, entry column uniform per wave), whose
    // writes all meet on one LDS bank (rows are 160 floats apart): 1.5 - 1.7 x slower in the cross shape
    static constexpr bool FAST_DEAL = FAST_DEAL_;
    static constexpr int SETS = CROSS ? 2 : 1;
    static constexpr int MT = R * WG;                // tiles a side per macro-tile
    static constexpr int ME = (O::TILES + MT - 1) / MT;
    static constexpr int MACROS = CROSS ? ME * ME : ME * (ME + 1) / 2;
    static constexpr int THREADS = 64 * WG * WG;
    static_assert(GRAM_SLAB % CHUNK == 0 && CHUNK % 4 == 0, "gram geometry");
    static_assert(O::SWZ_MASK == 0 || FAST_DEAL_, "the swizzle belongs to the deal by entry column");
};
using GramSym = GramShape<false, SCG_GRAM_R, SCG_GRAM_WG, SCG_GRAM_WPE, 64, false>;
using GramCross = GramShape<true, SCG_CROSS_GRAM_R, SCG_CROSS_GRAM_WG, 2, SCG_CROSS_GRAM_CHUNK, SCG_CROSS_GRAM_CP_FAST != 0>;
// SPEC §18's symmetric shape of order 3 or 7: GramSym's tiling, the deal by entry column (scg_basis.hip)
template <int ORDER_>
using GramBasis = GramShape<false, SCG_GRAM_R, SCG_GRAM_WG, SCG_GRAM_WPE, SCG_BASIS_GRAM_CHUNK, true, ORDER_>;
static_assert(GramSym::MT * 16 == SCG_GRAM_MACRO_TILE, "gram geometry");
static_assert(GramCross::MT * 16 == SCG_CROSS_GRAM_MACRO_TILE, "cross gram geometry");

// what the kernel forms next to A (its second template argument): nothing; b from one yv per sample, as column 0 of one more B operand;
// or SPEC §20.1's B from n_tgt <= GRAM_MAX_TGT targets per sample, which fill the 16 columns of that same operand
constexpr int GRAM_RHS_NONE = 0, GRAM_RHS_ONE = 1, GRAM_RHS_TARGETS = 2;
constexpr int GRAM_MAX_TGT = SCG_GRAM_MAX_TARGETS;
static_assert(GRAM_MAX_TGT == 16, "the targets are the columns of one 16-wide MFMA operand");

struct GramArgs {
    const float *s[2][4];                            // x, y, vx, vy of the row operands' states and of the column operands' (the same, or s2)
    const float *yv;                                 // yv and b: both or neither (GRAM_RHS_TARGETS: Y[n_tgt][y_stride] and B[seg][n_tgt][F])
    float *out, *b;                                  // A or C
    int32_t seg[GRAM_MAX_SEG];                       // the non-empty segments: index (A_g = out + seg * F^2), first sample, samples
    int64_t start[GRAM_MAX_SEG], count[GRAM_MAX_SEG];
    // GRAM_RHS_TARGETS only, and behind everything the other instantiations read: their code keeps its argument offsets
    int64_t y_stride;                                // floats between two targets' rows of Y (the entry point's n)
    int32_t n_tgt;
    // WEIGHTED only (SPEC §22.1), and behind everything else for the same reason
    const float *rw;                                 // the root weight of every sample
};
// grid = MACROS x n_active workgroups of THREADS on stream s (defined in scg_gram.hip); the first three read s[0] only
hipError_t launch_feature_gram(const GramArgs &G, int n_active, hipStream_t s);
hipError_t launch_feature_gram_targets(const GramArgs &G, int n_active, hipStream_t s);
hipError_t launch_feature_gram_weighted(const GramArgs &G, int n_active, hipStream_t s);      // G.n_tgt = 0: A only
hipError_t launch_feature_gram_irls(const GramArgs &G, int n_active, hipStream_t s);          // SPEC §23.2 at order 5: G.rw, G.yv = e, G.b = grad
hipError_t launch_feature_cross_gram(const GramArgs &G, int n_active, hipStream_t s);

// the table places of feature f (clamped: the tiles of a short macro-tile read a valid place and are never stored): AB at f / P2, CD
// behind them; `swz` is the reader lane's P1 s of GramOrder's swizzle (0 at order 5)
template <class O>
__device__ __forceinline__ void gram_places(int f, int swz, int &ab, int &cd) {
    f = min(f, O::F - 1);
    ab = (f / O::P2) ^ swz; cd = O::P2 + ((f % O::P2) ^ swz);
}
// phi_f of the sample whose table row is `row`, exactly as features_kernel forms it
__device__ __forceinline__ float gram_phi(const float2 *row, int ab_at, int cd_at) {
    const float2 ab = row[ab_at], cd = row[cd_at];
    return fmaf(-ab.y, cd.y, ab.x * cd.x);
}

// WEIGHTED (SPEC §22.1): every operand carries the sample's root weight, u_f(n) = rw[n] * phi_f(s_n) and t_c(n) = rw[n] * Y[c][n], one
// binary32 multiply each, so that A = sum rw^2 phi phi^T and B = sum rw^2 phi Y on §16.1's chains; both operands of a diagonal block
// carry it, so the block stays its own mirror image.
// IRLS (SPEC §23.2; with WEIGHTED and GRAM_RHS_ONE): A as WEIGHTED forms it, at any order, and b from the UNWEIGHTED phi against yv = e:
// the row operand's phi is kept beside its weighted copy, R more live registers per operand set, and only the b
// product reads it. yv carries no weight.
template <class S, int RHS, bool WEIGHTED = false, bool IRLS = false>
__global__ __launch_bounds__(S::THREADS, S::WPE) void gram_kernel(const GramArgs G) {
    constexpr bool CROSS = S::CROSS;
    constexpr int R = S::R, WG = S::WG, MT = S::MT, ME = S::ME, CHUNK = S::CHUNK, SETS = S::SETS, THREADS = S::THREADS;
    constexpr int P1 = S::P1, P2 = S::P2, F = S::F, TILES = S::TILES, TS = S::TS;
    constexpr bool TARGETS = RHS == GRAM_RHS_TARGETS;
    static_assert(RHS == GRAM_RHS_NONE || RHS == GRAM_RHS_ONE || TARGETS, "the three modes");
    static_assert(!(CROSS && RHS), "b belongs to the symmetric shape");
    static_assert(!TARGETS || (CHUNK % 16 == 0 && THREADS % 64 == 0), "the deal of the targets' fill");
    static_assert(!WEIGHTED || (!CROSS && (IRLS ? RHS == GRAM_RHS_ONE : (S::ORDER == 5 && RHS != GRAM_RHS_ONE))),
                  "the weighted shapes: symmetric; A alone or targets at order 5, or IRLS' one unweighted right-hand side at any order");
    static_assert(!IRLS || WEIGHTED, "IRLS is a weighted mode");
    __shared__ __attribute__((aligned(16))) float2 s_z1[SETS][CHUNK][4];
    __shared__ float2 s_tab[SETS][CHUNK * TS];
    // yv of the chunk; with TARGETS the chunk's targets sample-major, [CHUNK][16]: the B operand of four samples is 64 consecutive floats,
    // lane (n16, kk) reads its own bank (target-major rows of 64 floats would put the 16 lanes of a sample on one bank)
    __shared__ float s_yv[TARGETS ? CHUNK * GRAM_MAX_TGT : CHUNK];
    __shared__ float s_rw[WEIGHTED ? CHUNK : 1];               // WEIGHTED: the chunk's root weights, +0 for a null sample (else: never touched)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n16 = lane & 15, kk = lane >> 4;                 // MFMA operand lane: row / column n16 of the tile, k index (A, B) or row group (C, D)
    int I, J;                                                  // macro-tile (I, J)
    if (CROSS) { I = blockIdx.x / ME; J = blockIdx.x % ME; }   // the square row by row
    else {                                                     // I <= J: the upper triangle row by row
        int mj = blockIdx.x;
        for (I = 0; mj >= ME - I; ++I) mj -= ME - I;
        J = I + mj;
    }
    const int r0 = MT * I + R * (wave / WG), c0 = MT * J + R * (wave % WG);      // the wave's first row / column tile
    const bool diag = !CROSS && r0 == c0;                      // the block is its own mirror image
    // (the last macro-tile of a side is short; a block below the diagonal of the symmetric shape is the mirror image of one that is computed)
    const bool active = c0 < TILES && (CROSS ? r0 < TILES : r0 <= c0);
    const bool rhs = RHS && diag;                              // b's rows 16 r0 .. are this wave's
    int ra[R], rc[R], ca[R], cc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        gram_places<S>(16 * (r0 + r) + n16, P1 * (kk & S::SWZ_MASK), ra[r], rc[r]);
        gram_places<S>(16 * (c0 + r) + n16, P1 * (kk & S::SWZ_MASK), ca[r], cc[r]);
    }
    const f4v zero4 = (f4v){0.0f, 0.0f, 0.0f, 0.0f};
    f4v tot[R][R], acc[R][R], btot[R], bacc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        btot[r] = zero4; bacc[r] = zero4;
#pragma unroll
        for (int c = 0; c < R; ++c) { tot[r][c] = zero4; acc[r][c] = zero4; }
    }
    const int64_t first = G.start[blockIdx.y], count = G.count[blockIdx.y];
    for (int64_t s0 = 0; s0 < count; s0 += GRAM_SLAB) {
        const int slab = (int)(count - s0 < (int64_t)GRAM_SLAB ? count - s0 : (int64_t)GRAM_SLAB);
        for (int q0 = 0; q0 < slab; q0 += CHUNK) {
            const int m = min(CHUNK, slab - q0);               // samples of this chunk; its rows m .. up to the next multiple of 4 are null samples
            const int64_t base = first + s0 + q0;
            __syncthreads();                                   // the tables of the last chunk are consumed
            for (int t = tid; t < SETS * CHUNK * 4; t += THREADS) {
                const int set = CROSS ? t / (CHUNK * 4) : 0, smp = CROSS ? (t >> 2) % CHUNK : t >> 2, d = t & 3;
                if (smp < m) {
                    // (one table set: a select among four scalar registers; by index it is a load per chunk ahead of the state's)
                    const float *src = CROSS ? G.s[set][d] : (d == 0 ? G.s[0][0] : (d == 1 ? G.s[0][1] : (d == 2 ? G.s[0][2] : G.s[0][3])));
                    const float v = src[base + smp];
                    s_z1[set][smp][d] = sincospi_cs(d < 2 ? v : fmaf(v, 0.25f, 0.5f));     // state_powers' Z_d^1
                }
            }
            if (TARGETS) {
                // 16 consecutive samples of 4 targets per wave and pass: 64-byte runs of Y's rows from global memory, and the writes of a
                // wave meet 4 deep on 16 banks (one target per wave and pass: 16 deep on 4). +0 for a target >= n_tgt and a sample >= m
                for (int t = tid; t < CHUNK * GRAM_MAX_TGT; t += THREADS) {
                    const int smp = (t & 15) + 16 * (t >> 8), c = (t >> 4) & 15;
                    float v = c < G.n_tgt && smp < m ? G.yv[(int64_t)c * G.y_stride + base + smp] : 0.0f;
                    if constexpr (WEIGHTED) v = smp < m ? G.rw[base + smp] * v : 0.0f;       // t_c(n), rounded once
                    s_yv[smp * GRAM_MAX_TGT + c] = v;
                }
            } else if (RHS) {
                for (int t = tid; t < CHUNK; t += THREADS) s_yv[t] = t < m ? G.yv[base + t] : 0.0f;
            }
            if constexpr (WEIGHTED) {
                for (int t = tid; t < CHUNK; t += THREADS) s_rw[t] = t < m ? G.rw[base + t] : 0.0f;
            }
            __syncthreads();
            for (int t = tid; t < SETS * CHUNK * P1; t += THREADS) {
                const int set = CROSS ? t / (CHUNK * P1) : 0, u = CROSS ? t % (CHUNK * P1) : t;
                const int smp = S::FAST_DEAL ? u / P1 : u % CHUNK, cp = S::FAST_DEAL ? u % P1 : u / CHUNK;    // (slow deal: cp is wave-uniform)
                float2 *row = s_tab[set] + smp * TS;
                if (smp < m) {
                    float2 ab[P1], cd[P1];
                    item_entries(&s_z1[set][smp][0], cp, ab, cd);
                    const int wz = P1 * (smp & S::SWZ_MASK);   // (0 at order 5)
#pragma unroll
                    for (int c = 0; c < P1; ++c) { row[(P1 * c + cp) ^ wz] = ab[c]; row[P2 + ((P1 * c + cp) ^ wz)] = cd[c]; }
                } else if (smp < ((m + 3) & ~3)) {
#pragma unroll
                    for (int c = 0; c < P1; ++c) { row[P1 * c + cp] = make_float2(0.0f, 0.0f); row[P2 + P1 * c + cp] = make_float2(0.0f, 0.0f); }
                }
            }
            __syncthreads();
            if (active) {
                // per four samples: the operands of the NEXT four are read and formed before this four's products are issued (one wave per
                // SIMD: nothing else hides the LDS round trip); a full chunk's loop is unrolled, a short one runs the same steps
                const float2 *rowa = s_tab[0] + kk * TS, *rowb = s_tab[SETS - 1] + kk * TS;
                constexpr int RU = IRLS ? R : 1;                 // IRLS: the row operands' unweighted phi, for b
                float a[R], bo[R], an[R], bn[R], au[RU], aun[RU];
                auto operands = [&](int ks, float (&pa)[R], float (&pb)[R], float (&pu)[RU]) {
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        pa[r] = gram_phi(rowa + 4 * ks * TS, ra[r], rc[r]);
                        pb[r] = gram_phi(rowb + 4 * ks * TS, ca[r], cc[r]);
                    }
                    if constexpr (WEIGHTED) {                         // u = rw * phi: a multiply of its own behind gram_phi's fma, 2 R per R^2 MFMAs
                        const float w = s_rw[4 * ks + kk];
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            if constexpr (IRLS) pu[r] = pa[r];
                            pa[r] = w * pa[r]; pb[r] = w * pb[r];
                        }
                    }
                };
                auto step = [&](int ks, bool more) {
                    if (more) operands(ks + 1, an, bn, aun);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
#pragma unroll
                        for (int c = 0; c < R; ++c) acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], bo[c], acc[r][c], 0, 0, 0);
                    }
                    if (rhs) {                                 // yv as column 0 of a B operand: column 0 of the product is b's chain
                        // (TARGETS: target c as column c; a column of the product depends on that column of the operand only)
                        const float yb = TARGETS ? s_yv[(4 * ks + kk) * GRAM_MAX_TGT + n16] : (n16 == 0 ? s_yv[4 * ks + kk] : 0.0f);
#pragma unroll
                        for (int r = 0; r < R; ++r) bacc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(IRLS ? au[r] : a[r], yb, bacc[r], 0, 0, 0);
                    }
#pragma unroll
                    for (int r = 0; r < R; ++r) { a[r] = an[r]; bo[r] = bn[r]; if constexpr (IRLS) au[r] = aun[r]; }
                };
                operands(0, a, bo, au);
                if (m == CHUNK) {
#pragma unroll
                    for (int ks = 0; ks < CHUNK / 4; ++ks) step(ks, ks + 1 < CHUNK / 4);
                } else {
                    const int nks = (m + 3) >> 2;
                    for (int ks = 0; ks < nks; ++ks) step(ks, ks + 1 < nks);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {                          // the slab's P joins the segment's total; the next slab starts from +0
            btot[r] = btot[r] + bacc[r]; bacc[r] = zero4;
#pragma unroll
            for (int c = 0; c < R; ++c) { tot[r][c] = tot[r][c] + acc[r][c]; acc[r][c] = zero4; }
        }
    }
    if (!active) return;
    // accumulator lane (n16, kk), register v = entry (row 4 kk + v, column n16) of the tile
    float *Og = G.out + (size_t)G.seg[blockIdx.y] * F * F;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (r0 + r >= TILES) continue;
        const int row = 16 * (r0 + r) + 4 * kk;
#pragma unroll
        for (int c = 0; c < R; ++c) {
            if (c0 + c >= TILES) continue;
            const int col = 16 * (c0 + c) + n16;
#pragma unroll
            for (int v = 0; v < 4; ++v) Og[(size_t)(row + v) * F + col] = tot[r][c][v];
            if (!CROSS && !diag) {                             // the mirror image (a diagonal block holds its own)
#pragma unroll
                for (int v = 0; v < 4; ++v) Og[(size_t)col * F + row + v] = tot[r][c][v];
            }
        }
        if (TARGETS) {
            if (rhs && n16 < G.n_tgt) {                        // column n16 is target n16's; the lanes of the zero columns store nothing
#pragma unroll
                for (int v = 0; v < 4; ++v) G.b[((size_t)G.seg[blockIdx.y] * G.n_tgt + n16) * F + row + v] = btot[r][v];
            }
        } else if (rhs && n16 == 0) {
#pragma unroll
            for (int v = 0; v < 4; ++v) G.b[(size_t)G.seg[blockIdx.y] * F + row + v] = btot[r][v];
        }
    }
}
