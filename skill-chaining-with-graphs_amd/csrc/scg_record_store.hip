// scg_record_store.hip — SPEC §30.1: the device record store. record_append_kernel (a launch's [rows][n] buffers behind each env's
// earlier rows in [n][cap] arrays: a transposing copy through LDS) with record_commit_kernel (the per-env counts), record_offsets_kernel
// (the exclusive scan of the counts) and record_pack_kernel (the store's rows as the flat (env, row) record, with the row tables of the
// value fits), and their launches.
//
// A unit of its own for the reason scg_returns.hip gives: what shares a module with a kernel may change that kernel's gfx950 code,
// and here nothing can. The entry points and their checks are in scg_kernels.hip. Nothing here computes: every kernel moves bytes,
// selects, or adds integers, so the bits do not depend on the block build or the launch geometry.
#include "scg_device.hpp"
#include "../../include/scg_abi.h"

#include "scg_record_store.hpp"

static_assert(RS_WAVES * 64 == 4 * RS_TILE && RS_TILE == 64, "a tile row (and a tile column) is one wave wide");

__device__ __forceinline__ int clamp_i32(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// ------------------------------------------------------------------ append
// One field of one tile. In: wave w takes the launch rows r0 + w, r0 + w + 4, ..., lane = env: 64 consecutive elements of a launch row,
// one coalesced load. Out: wave w takes the envs e0 + w, e0 + w + 4, ..., lane = row: 64 consecutive elements of the env's store range,
// one coalesced store. In between the tile lies in LDS as 32-bit words at a row stride of 65: the row-wise write puts a wave's lanes
// into consecutive words, the column-wise read into words 65 apart: ds_write_b32 and ds_read_b32 bank by (a / 4) % 32 within each
// 32-lane half, and either way a half's lanes fall into 32 different banks (at a stride of 64 words the column read would be a
// 32-way conflict). A 1-byte field is widened to a word on the way in and narrowed on the way out, so that it takes the same
// conflict-free path (a byte tile would put four of a column's rows into one word). Elements at or beyond an env's len were not written by the launch and are neither loaded nor stored.
template <typename T>
__device__ __forceinline__ void append_field(const RecordAppendArgs &A, const RecordFieldPair &f, uint32_t (*tile)[RS_PAD],
                                             const int *s_len, const int *s_have, int e0, int r0, int lane, int wave) {
    const T *src = static_cast<const T *>(f.src);
    T *dst = static_cast<T *>(f.dst);
    const int e_in = e0 + lane;
#pragma unroll 4
    for (int rr = wave; rr < RS_TILE; rr += RS_WAVES) {
        const int r = r0 + rr;
        if (e_in < A.n && r < s_len[lane]) {                   // (len <= rows: r is a row of the launch)
            const T v = src[(int64_t)r * A.n + e_in];
            tile[rr][lane] = (uint32_t)v;                      // (T is uint32_t or uint8_t: a 4-byte field moves as its bits)
        }
    }
    __syncthreads();
    const int r_out = r0 + lane;
#pragma unroll 4
    for (int ee = wave; ee < RS_TILE; ee += RS_WAVES) {
        const int e = e0 + ee;
        const int64_t at = (int64_t)s_have[ee] + r_out;        // the row's place in the env's range; rows that pass cap are dropped
        if (e < A.n && r_out < s_len[ee] && at < A.cap) {
            dst[(int64_t)e * A.cap + at] = (T)tile[lane][ee];
        }
    }
    __syncthreads();                                           // the tile is rewritten by the next field
}

// grid (env tiles, row tiles). Reads have, never writes it: every row tile of an env places its rows from the same count.
__global__ __launch_bounds__(RS_WAVES * 64) void record_append_kernel(const RecordAppendArgs A) {
    __shared__ uint32_t tile[RS_TILE][RS_PAD];
    __shared__ int s_len[RS_TILE], s_have[RS_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int e0 = blockIdx.x * RS_TILE, r0 = blockIdx.y * RS_TILE;
    if (tid < RS_TILE) {
        const int e = e0 + tid;
        s_len[tid] = e < A.n ? clamp_i32(A.len[e], A.rows) : 0;
        s_have[tid] = e < A.n ? clamp_i32(A.have[e], A.cap) : 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RS_FIELDS; ++k) {
        if (!A.f[k].src || !A.f[k].dst) continue;              // (uniform over the grid)
        if (k < 5) append_field<uint32_t>(A, A.f[k], tile, s_len, s_have, e0, r0, lane, wave);
        else append_field<uint8_t>(A, A.f[k], tile, s_len, s_have, e0, r0, lane, wave);
    }
}

// have[e] += len[e], stopping at cap; the rows that did not fit are counted. Launched behind record_append_kernel on its stream.
__global__ __launch_bounds__(RS_WAVES * 64) void record_commit_kernel(const RecordAppendArgs A) {
    const int e = blockIdx.x * (RS_WAVES * 64) + threadIdx.x;
    if (e >= A.n) return;
    const int64_t want = (int64_t)clamp_i32(A.have[e], A.cap) + clamp_i32(A.len[e], A.rows);
    const int64_t now = want < A.cap ? want : A.cap;
    A.have[e] = (int32_t)now;
    if (want > now) atomicAdd(A.overflow, (int)(want - now));  // (an integer count: its order does not matter)
}

hipError_t launch_record_append(const RecordAppendArgs &A, hipStream_t s) {
    const dim3 grid((A.n + RS_TILE - 1) / RS_TILE, (A.rows + RS_TILE - 1) / RS_TILE);
    hipLaunchKernelGGL(record_append_kernel, grid, dim3(RS_WAVES * 64), 0, s, A);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(record_commit_kernel, dim3((A.n + RS_WAVES * 64 - 1) / (RS_WAVES * 64)), dim3(RS_WAVES * 64), 0, s, A);
    return hipGetLastError();
}

// ------------------------------------------------------------------ offsets
// offsets[e] = have[0] + ... + have[e - 1] in int64, offsets[n] the total: one workgroup walks the counts in chunks of 1024 with the
// running total in a register; a chunk is scanned by shuffles inside each wave and the sixteen wave totals through LDS.
constexpr int RO_THREADS = 1024;

__global__ __launch_bounds__(RO_THREADS) void record_offsets_kernel(int32_t n, const int32_t *have, int64_t *offsets) {
    __shared__ long long s_wave[RO_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long carry = 0;
    for (int64_t base = 0; base < n; base += RO_THREADS) {
        const int64_t i = base + tid;
        const long long v = i < n ? (long long)have[i] : 0;
        long long inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long t = __shfl_up(inc, d, 64);
            if (lane >= d) inc += t;
        }
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        long long before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < RO_THREADS / 64; ++w) {
            const long long t = s_wave[w];
            before += w < wave ? t : 0;
            all += t;
        }
        if (i < n) offsets[i] = carry + before + inc - v;
        carry += all;
        __syncthreads();                                       // the wave totals are rewritten by the next chunk
    }
    if (tid == 0) offsets[n] = carry;
}

hipError_t launch_record_offsets(int32_t n, const int32_t *have, int64_t *offsets, hipStream_t s) {
    hipLaunchKernelGGL(record_offsets_kernel, dim3(1), dim3(RO_THREADS), 0, s, n, have, offsets);
    return hipGetLastError();
}

// ------------------------------------------------------------------ pack
// One wave per env, its rows in steps of 64: lane = row, so the store side (the env's range) and the flat side (offsets[e] onwards) are
// both consecutive. The env's flat range is clamped as the scans clamp it (scg_returns.hip) and cut to cap rows, so that no offsets
// make the kernel read outside the store or write outside [0, total). The tables are SPEC §30.1's, formed from the store's bytes:
// tabA reads vf of the row behind where that row is the env's.
__global__ __launch_bounds__(RS_WAVES * 64) void record_pack_kernel(const RecordPackArgs A) {
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * RS_WAVES + (threadIdx.x >> 6);
    if (e >= A.n) return;                                      // (wave-uniform)
    int64_t lo = A.offsets[e], hi = A.offsets[e + 1];
    lo = lo < 0 ? 0 : (lo > A.total ? A.total : lo);           // no offsets reach outside [0, total)
    hi = hi < lo ? lo : (hi > A.total ? A.total : hi);
    const int64_t L = hi - lo < A.cap ? hi - lo : A.cap;       // ... or outside the env's range of the store
    const int64_t s0 = e * A.cap;
    const bool tables = A.tab0 || A.tabk || A.tabA;
    for (int64_t r = lane; r < L; r += 64) {
        const int64_t i = lo + r, s = s0 + r;
#pragma unroll
        for (int k = 0; k < RS_FIELDS; ++k) {
            if (!A.f[k].src || !A.f[k].dst) continue;          // (uniform over the grid)
            if (k < 5) static_cast<uint32_t *>(A.f[k].dst)[i] = static_cast<const uint32_t *>(A.f[k].src)[s];
            else static_cast<uint8_t *>(A.f[k].dst)[i] = static_cast<const uint8_t *>(A.f[k].src)[s];
        }
        if (A.env) A.env[i] = (int32_t)e;
        if (A.row) A.row[i] = (int32_t)r;
        if (tables) {
            const int dn = A.done[s], o = A.vf[s], tm = A.term[s];
            if (A.tab0) A.tab0[i] = dn == 0 ? 0 : SCG_ROW_NONE;
            if (A.tabk) A.tabk[i] = (o >= 1 && tm == 0 && dn == 0) ? (uint8_t)o : SCG_ROW_NONE;
            if (A.tabA) A.tabA[i] = (r + 1 < L && (r == 0 || dn == 0)) ? A.vf[s + 1] : SCG_ROW_NONE;
        }
    }
}

hipError_t launch_record_pack(const RecordPackArgs &A, hipStream_t s) {
    hipLaunchKernelGGL(record_pack_kernel, dim3((A.n + RS_WAVES - 1) / RS_WAVES), dim3(RS_WAVES * 64), 0, s, A);
    return hipGetLastError();
}
