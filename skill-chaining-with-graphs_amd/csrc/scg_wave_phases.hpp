// scg_wave_phases.hpp — the launch geometry and the per-step phases that rollout_kernel and trial_kernel share (included by
// scg_rollout_kernel.hpp, and by scg_trial_kernel.hpp through it). A workgroup of RO_WAVES waves owns RO_WAVES * epw consecutive
// envs / entries, one per lane (lanes < epw); each wave has a private table area of RO_WAVE_FLOATS floats in LDS.
// Everything here is __forceinline__: the two kernels sit at 183 .. 235 VGPRs without scratch, and DESIGN §3.8–3.11 records what a
// live pointer or the record taken by reference costs them. NOT here: the E loop (folded, it cost every instantiation
// one or two VGPRs), SPEC §10's row store and SPEC §9's end code (folded, they changed the code of four instantiations).
#pragma once

constexpr int RO_WAVES = 8;                    // waves per workgroup
constexpr int RO_THREADS = RO_WAVES * 64;
constexpr int RO_MAX_EPW = 32;                 // envs per wave (launch parameter epw in 2..32, a power of two)
constexpr int RO_MAX_ENVS = RO_WAVES * RO_MAX_EPW;
constexpr int RO_WAVE_FLOATS = E_TAB_FLOATS;   // per wave: tables of one unit (E) / the physics' pair list + states (P)
static_assert(PITEMS + 4 * 64 + 16 <= RO_WAVE_FLOATS, "the pair list, the states and the goal flags fit a wave's table area");
static_assert(RO_MAX_ENVS <= 256, "list entries are 8-bit env indices");

// the kernel arguments through an opaque copy of the argument pointer: the record's pointers are fetched at the store site this
// way, and the outputs at the exit; kept live from the entry they would sit in scalar registers across the whole step loop, where
// they crowd the loop's own scalars out into spill slots
template <typename Args>
__device__ __forceinline__ const Args *kernel_args() {
    const Args *K = (const Args *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(K));
    return K;
}

// ------------------------------------------------------------------ SPEC §10's record
// The record is taken BY VALUE wherever it is read: through a reference the compiler cannot tell the record's own stores from the
// kernel arguments and reloads every pointer after each store, one memory round trip at a time.
// len of env e (0: skipped) when e lies in the record's window
__device__ __forceinline__ void record_len(const scg_record R, int e, bool mine, int len) {
    const int r = e - R.first;
    if (mine && r >= 0 && r < R.n) R.len[r] = len;
}

// ------------------------------------------------------------------ P
// One Pinball step of the wave's envs (lanes with `phys`) on the wave's own (env, edge) pair list, carved out of its table area
// `sw`: the pair list, the states and the goal flags. (wave-uniform call.) Returns the reward; the state and `goal` are s'
__device__ __forceinline__ float wave_physics(const float *s_edges, const uint64_t *cellmask, const MapScalars &ms, float *sw, bool phys,
                                              float &x, float &y, float &vx, float &vy, int a, bool &goal) {
    uint32_t *items = reinterpret_cast<uint32_t *>(sw);
    float *xs = sw + PITEMS;
    uint8_t *gfl = reinterpret_cast<uint8_t *>(sw + PITEMS + 4 * 64);
    bool pr;                                               // the pair parity: prepare's, for finish
    const int groups = pinball_wave_prepare_any(s_edges, cellmask, ms, phys, x, y, vx, vy, a, goal, pr, items, xs, 64);
    wave_lds_sync();
    for (int q = 0; q < groups; ++q) pinball_wave_group(s_edges, ms, items + 64 * q, xs, 64, gfl);
    wave_lds_sync();
    return pinball_wave_finish(pr, x, y, vx, vy, a, goal, xs, 64, gfl);
}
// Z_d^1 of a state, d = 0..3
__device__ __forceinline__ void store_z1(float2 *dst, float x, float y, float vx, float vy) {
    const float sh[4] = {x, y, fmaf(vx, 0.25f, 0.5f), fmaf(vy, 0.25f, 0.5f)};
#pragma unroll
    for (int d = 0; d < 4; ++d) dst[d] = sincospi_cs(sh[d]);
}
// The wave's lanes with `pred` append `value` to the list behind the LDS counter *ctr: ballot / popcount, one atomic per wave.
// (wave-uniform call.)
__device__ __forceinline__ void list_append(int *ctr, uint16_t *list, bool pred, uint16_t value, int lane) {
    const uint64_t b = __ballot(pred);
    if (!b) return;                                        // (wave-uniform)
    int base = 0;
    if (lane == 0) base = atomicAdd(ctr, __popcll(b));
    base = __shfl(base, 0, 64);
    if (pred) list[base + __popcll(b & ((1ull << lane) - 1ull))] = value;
}
