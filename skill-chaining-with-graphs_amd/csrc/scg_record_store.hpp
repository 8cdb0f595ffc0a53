// scg_record_store.hpp — SPEC §30.1: the arguments and the launches of the device record store's kernels (all compiled in
// scg_record_store.hip; scg_kernels.hip includes this header for the entry points' wrappers and holds no code of the kernels).
#pragma once

constexpr int RS_TILE = 64;                    // a transposed tile: RS_TILE launch rows x RS_TILE envs
constexpr int RS_PAD = RS_TILE + 1;            // its LDS row stride in 32-bit words: a column read falls into 32 different banks per 32-lane half
constexpr int RS_WAVES = 4;                    // waves per workgroup of every kernel here
constexpr int RS_FIELDS = 10;                  // scg_record's fields: five of 4 bytes (x, y, vx, vy, reward), then five of 1 byte

// One field on both sides of a copy; null on either side: skipped.
struct RecordFieldPair {
    const void *src;
    void *dst;
};

struct RecordAppendArgs {
    RecordFieldPair f[RS_FIELDS];  // src [rows][n] (the launch buffers), dst [n][cap] (the store); 0 .. 4 of 4 bytes, 5 .. 9 of 1 byte
    const int32_t *len;            // [n] rows the launch wrote per env (clamped into [0, rows] by the kernels)
    int32_t *have;                 // [n] rows the store holds per env (read clamped into [0, cap]); written by the commit kernel only
    int32_t *overflow;             // [1] rows dropped so far
    int32_t n, rows, cap;
};

struct RecordPackArgs {
    RecordFieldPair f[RS_FIELDS];  // src [n][cap] (the store), dst [total] (the flat record)
    const uint8_t *done, *vf, *term;   // the store's, for the tables (null where no table is asked for)
    const int64_t *offsets;        // [n + 1] env e owns flat rows offsets[e] .. offsets[e + 1] - 1 (clamped into [0, total]; at most cap rows)
    int32_t *env, *row;            // [total] each flat row's env and local row (null: not written)
    uint8_t *tab0, *tabk, *tabA;   // [total] SPEC §30.1's tables (null: not written)
    int64_t total;
    int32_t n, cap;
};

hipError_t launch_record_append(const RecordAppendArgs &A, hipStream_t s);                          // n, rows, cap >= 1
hipError_t launch_record_offsets(int32_t n, const int32_t *have, int64_t *offsets, hipStream_t s);  // n >= 0
hipError_t launch_record_pack(const RecordPackArgs &A, hipStream_t s);                              // n >= 1, total >= 1
