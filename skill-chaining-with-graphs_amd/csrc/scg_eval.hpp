// scg_eval.hpp — the E unit shared by td_kernel and rollout_kernel (included by scg_kernels.hip): Q(s, .) of 8 items of one value
// function from their Z_d^1, in SPEC §3.1's summation order (the CPU oracle reproduces every bit).
//   tables  per item: CDk[c34][col] and ABq[col][c12] with ABsel = (Re AB | -Im AB), in the calling wave's private table area
//   T       W_k (180 x 36) x [Re CD | Im CD] on v_mfma_f32_16x16x4_f32, W_k the A operand: from LDS in the A-operand layout, or
//           straight from memory
//   fold    per action, T's rows against the AB factors, row tiles in order, then the butterfly over the item's 16 partial sums
// Lane roles. As an MFMA operand lane (16x16x4): n16 = lane & 15 is the tile row (A) / column (B, C, D), g = lane >> 4
// the k index (A, B) / the row group (C, D: rows 4 g + v). As a table builder: bi = lane & 7 is the item of an
// 8-item column block, cp = lane >> 3 the second index (c2 / c4; lanes with cp >= 6 idle).
// Columns of an 8-item block: item j = 4 h + i  (h = 0, 1; i = 0..3) has its real-part column at 8 h + i and its
// imaginary-part column at 8 h + 4 + i.
#pragma once

// A-operand layout of W_k: 12 row tiles x 9 k-blocks x 64 lanes; per tile and lane the k-blocks 0..3 and 4..7 form two float4
// (float4 d: tile d >> 7, k-blocks 4 ((d >> 6) & 1) .., lane d & 63) — one ds_read_b128 feeds four MFMAs — and k-block 8 of every
// tile sits behind them (float W_TAIL + z: tile z >> 6, lane z & 63)
constexpr int W_FLOATS = 12 * 9 * 64;
constexpr int W_TAIL = 12 * 2 * 64 * 4;
constexpr int AS = 40;                                         // row stride of ABq (floats): the fold's ds_read_b128 conflict-free
constexpr int E_TAB_FLOATS = 36 * 16 + 16 * AS;                // one wave's tables: CDk[36][16], ABq[16][AS]
// row tiles per operand group (contract_with's TG), settled by A/Bs of both kernels (the rollout at 65 536 envs: 4 or 6 tiles from
// memory instead of 3 ran 1.8 % / 14 % slower, all twelve tiles from both sources 16 %)
constexpr int E_TG = 4;                                        // ... of the LDS-fed contraction
constexpr int EO_TG = 3;                                       // ... of the contraction from memory (register budget: 9 per tile)

// four floats from a 4-byte-aligned address, as one 16-byte load
__device__ __forceinline__ f4v load4_unaligned(const float *p) {
    struct __attribute__((packed, aligned(4))) F4U { float x, y, z, w; };
    const F4U u = *reinterpret_cast<const F4U *>(p);
    return (f4v){u.x, u.y, u.z, u.w};
}

// entry (tile t, k-block kb, lane ln) of the A-operand layout = W_k[16 t + (ln & 15)][9 (ln >> 4) + kb] = W_k[src]; rows >= 180 are zeros (false)
__device__ __forceinline__ bool w_a_src(int t, int kb, int ln, int &src) {
    const int row = 16 * t + (ln & 15);
    src = row * 36 + 9 * (ln >> 4) + kb;
    return row < NACT * 36;
}

// ------------------------------------------------------------------ SPEC §3 tables of one item
// AB[c2] = Z_1^c2, AB[c1*6 + c2] = cmul(AB[(c1-1)*6 + c2], Z_0^1) (CD likewise from Z_3, Z_2), Z^0 = (1, 0), Z^k = cmul(Z^(k-1), Z^1):
// five chained products per table column instead of a power chain plus a product per entry.
// (P1 = order + 1 entries a table row: 6 everywhere but in SPEC §18's basis-order probe, whose Gram kernel builds rows of 4 and 8)
template <int P1>
__device__ __forceinline__ float2 zpow_sel(float2 z, int c) {
    float2 cur = z, out = make_float2(1.0f, 0.0f);
#pragma unroll
    for (int j = 1; j <= P1 - 1; ++j) {
        if (c == j) out = cur;
        if (j < P1 - 1) cur = cmul(cur, z);
    }
    return out;
}
// from the item's four Z_d^1 (z1p: 4 float2 in LDS) the lane with second index `cp` (c2 of AB, c4 of CD; cp < 6) gets, for the
// first index c = 0..5, AB[6c + cp] and CD[6c + cp] (P1 is deduced from the arrays: 6 here)
template <int P1>
__device__ __forceinline__ void item_entries(const float2 *z1p, int cp, float2 (&ab)[P1], float2 (&cd)[P1]) {
    const float4 za = *reinterpret_cast<const float4 *>(z1p), zc = *reinterpret_cast<const float4 *>(z1p + 2);
    const float2 z0 = make_float2(za.x, za.y), z1 = make_float2(za.z, za.w);
    const float2 z2 = make_float2(zc.x, zc.y), z3 = make_float2(zc.z, zc.w);
    ab[0] = zpow_sel<P1>(z1, cp); cd[0] = zpow_sel<P1>(z3, cp);
#pragma unroll
    for (int c = 1; c < P1; ++c) {
        ab[c] = cmul(ab[c - 1], z0);
        cd[c] = cmul(cd[c - 1], z2);
    }
}
// the builder lane's share of one 8-item column block's tables (item at z1p, real-part column bcol)
__device__ __forceinline__ void build_tables(const float2 *z1p, int cp, int bcol, float *cdk, float *abq) {
    if (cp < 6) {
        float2 ab[6], cd[6];
        item_entries(z1p, cp, ab, cd);
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            abq[bcol * AS + 6 * c + cp] = ab[c].x; abq[(bcol + 4) * AS + 6 * c + cp] = -ab[c].y;
            cdk[(6 * c + cp) * 16 + bcol] = cd[c].x; cdk[(6 * c + cp) * 16 + bcol + 4] = cd[c].y;
        }
    }
}
// the B operand of operand lane (n16, g): [Re CD | Im CD] rows 9 g .. 9 g + 8 of column n16
__device__ __forceinline__ void load_b(const float *cdk, int n16, int g, float (&B)[9]) {
#pragma unroll
    for (int kb = 0; kb < 9; ++kb) B[kb] = cdk[(9 * g + kb) * 16 + n16];
}

// SPEC §3.1 butterfly over the 16 partial sums of one item (4 row groups x re|im, the item's 8 columns hold
// [re x 4 items, im x 4 items]): u_g = q_re + q_im (lane xor 4), then (u_0 + u_1) + (u_2 + u_3) (lane xor 16, 32)
template <int M>
__device__ __forceinline__ void item_tree_sum(float (&q)[M]) {
#pragma unroll
    for (int a = 0; a < M; ++a) q[a] = q[a] + swz_xor4(q[a]);
#pragma unroll
    for (int a = 0; a < M; ++a) {
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(q[a]), __float_as_uint(q[a]), false, false);
        q[a] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
#pragma unroll
    for (int a = 0; a < M; ++a) {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(q[a]), __float_as_uint(q[a]), false, false);
        q[a] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
}

// ------------------------------------------------------------------ SPEC §3.1 contraction
// Q(sigma, .) of the 8 items whose B operand and AB factors (ab_lane = ABq + n16 AS + 4 g) the wave holds: T = W (180 x 36) x
// [Re CD | Im CD] on the matrix pipe — rows 16 t + 4 g + v -> action rho / 36, c12 = rho % 36; a lane's four rows never straddle
// actions — then the fold with the AB factors and the butterfly. The twelve row tiles are taken in groups of TG (MFMAs, then the
// fold of those TG accumulators into the per-action chains, tile order kept): 4 TG accumulator registers instead of 48.
// load_a(t, a0, a1, a8) fetches tile t's A operands (k-blocks 0..3, 4..7, 8). The finished sums are in the lanes with
// g == 0 and !(n16 & 4) (item 4 (n16 >> 3) + (n16 & 3)).
template <int TG, typename LoadA>
__device__ __forceinline__ void contract_with(LoadA load_a, const float (&B)[9], float (&qo)[NACT], int g, const float *ab_lane) {
    static_assert(12 % TG == 0, "whole tile groups");
    float q[NACT + 1] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    // the operands of group hh + 1 are fetched before the products of group hh are issued (two operand sets in registers)
    f4v a0[2][TG], a1[2][TG];
    float a8[2][TG];
#pragma unroll
    for (int tt = 0; tt < TG; ++tt) load_a(tt, a0[0][tt], a1[0][tt], a8[0][tt]);
#pragma unroll
    for (int hh = 0; hh < 12 / TG; ++hh) {
        if (hh + 1 < 12 / TG) {
#pragma unroll
            for (int tt = 0; tt < TG; ++tt) load_a(TG * (hh + 1) + tt, a0[(hh + 1) & 1][tt], a1[(hh + 1) & 1][tt], a8[(hh + 1) & 1][tt]);
        }
        f4v acc[TG];
#pragma unroll
        for (int tt = 0; tt < TG; ++tt) {
            f4v c = (f4v){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[hh & 1][tt][kb], B[kb], c, 0, 0, 0);
#pragma unroll
            for (int kb = 0; kb < 4; ++kb) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[hh & 1][tt][kb], B[4 + kb], c, 0, 0, 0);
            acc[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a8[hh & 1][tt], B[8], c, 0, 0, 0);
        }
#pragma unroll
        for (int tt = 0; tt < TG; ++tt) {
            const int t = TG * hh + tt;
            const int Ct = (16 * t) % 36, At = (16 * t) / 36;
            if (Ct + 12 < 36) {                          // the tile's 16 rows belong to one action
                const f4v ab4 = *reinterpret_cast<const f4v *>(ab_lane + Ct);
#pragma unroll
                for (int vv = 0; vv < 4; ++vv) q[At] = fmaf(acc[tt][vv], ab4[vv], q[At]);
            } else {                                     // row groups g >= (36 - Ct) / 4 belong to the next action
                const bool wrap = 4 * g >= 36 - Ct;
                const f4v ab4 = *reinterpret_cast<const f4v *>(ab_lane + (wrap ? Ct - 36 : Ct));
                float xq = wrap ? q[At + 1] : q[At];
#pragma unroll
                for (int vv = 0; vv < 4; ++vv) xq = fmaf(acc[tt][vv], ab4[vv], xq);
                q[At] = wrap ? q[At] : xq;
                q[At + 1] = wrap ? xq : q[At + 1];
            }
        }
    }
#pragma unroll
    for (int a = 0; a < NACT; ++a) qo[a] = q[a];
    item_tree_sum<NACT>(qo);
}
// ... A operands from a W_k staged in the A-operand layout at float offset `wofs` of an LDS area whose float4 / float at this
// lane's place are w4 / w8 (two ds_read_b128 + one ds_read_b32 per tile)
template <int TG>
__device__ __forceinline__ void contract_lds(int wofs, const float (&B)[9], float (&qo)[NACT], int g, const f4v *w4, const float *w8,
                                             const float *ab_lane) {
    contract_with<TG>([&](int t, f4v &a0, f4v &a1, float &a8) {
        a0 = w4[wofs / 4 + (t * 2) * 64]; a1 = w4[wofs / 4 + (t * 2 + 1) * 64]; a8 = w8[wofs + t * 64];
    }, B, qo, g, ab_lane);
}
// ... A operands straight from W_k[5][36][36] in memory: lane (n16, g) of tile t owns the nine consecutive floats
// W[16 t + n16][9 g .. 9 g + 8] (two 16-byte loads at 4-byte-aligned addresses and one float; rows >= 180: zeros)
template <int TG>
__device__ __forceinline__ void contract_mem(const float *Wk, const float (&B)[9], float (&qo)[NACT], int n16, int g, const float *ab_lane) {
    contract_with<TG>([&](int t, f4v &a0, f4v &a1, float &a8) {
        const int row = 16 * t + n16;
        a0 = (f4v){0.0f, 0.0f, 0.0f, 0.0f}; a1 = a0; a8 = 0.0f;
        if (row < NACT * 36) {
            const float *pw = Wk + row * 36 + 9 * g;
            a0 = load4_unaligned(pw); a1 = load4_unaligned(pw + 4); a8 = pw[8];
        }
    }, B, qo, g, ab_lane);
}
