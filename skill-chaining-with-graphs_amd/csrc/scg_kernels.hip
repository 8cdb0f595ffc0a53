// scg_kernels.hip — the C-ABI of include/scg_abi.h: the context, its helpers and the entry points, which launch the gfx950 kernels of the
// headers included below. All of them are compiled HERE, in one module and in this order (what shares a module
// with the hot kernels changes their code); the host code stays in this file because it launches them.
//   scg_device.hpp           constants, Pinball physics, Fourier factors, classifier — shared by every kernel
//   scg_eval.hpp             the per-env step and the E unit shared by the step, rollout and trial kernels
//   scg_step_kernel.hpp      StepArgs + td_kernel: one step-batch (SPEC §5) = td_kernel<FUSED> -> the reduce launch. A workgroup = 16
//                            wavefronts owns 256 consecutive positions of the option-sorted env order and the whole LDS of its CU
//   scg_wave_phases.hpp      the rollout / trial launch geometry and the phases the two kernels share (included by the next header)
//   scg_rollout_kernel.hpp   rollout_kernel: K acting steps (SPEC §8) in one launch, a fixed range of envs per workgroup
//   scg_trial_kernel.hpp     trial_kernel: option trials (SPEC §9) with the rollout's geometry
//   scg_order.hpp            SPEC §5 env order: sort key, layout of the option runs, the stand-alone sort (sort_hist / sort_scatter,
//                            run when no env order is prepared)
//   scg_collect_kernels.hpp  SPEC §7 / §13: harvest, collect and frontier kernels
//   scg_reduce_kernel.hpp    reduce_kernel: slabs -> 16-block segment sums -> G, n_k, W += alpha/n_k * scale * G; commit + next env
//                            order (+ an announced example trigger's row totals); commit_kernel for acting-only steps
//   scg_apply_kernels.hpp    the update outside the reduce launch: one operand, slots in order, the peer transport
//   scg_aux_kernels.hpp      pinball / features / predict, and fit_kernel: SPEC §6 on 8 workgroups x 1024 chains per option behind
//                            tagged-word exchanges; a fit whose workgroups cannot run together gives up after a wall-clock wait,
//                            leaves its row untouched and raises the ctx's asynchronous status word
//   scg_gram_kernel.hpp      SPEC §16.1's feature Gram, §20.1's with up to 16 right-hand sides, §22.1's weighted one and §17.1's cross-feature Gram, one kernel
//                            template (and §23.2's IRLS mode of it): here only its arguments and the five launches (its instantiations are
//                            compiled in scg_gram.hip)
//   scg_basis_kernels.hpp    SPEC §18's basis-order probe, §23's logistic terms and IRLS Gram at the orders 3 and 7 and §24.2's
//                            classifier logits: here only the launches (compiled in scg_basis.hip)
// scg_rollout_variants.hip is the second translation unit: every other instantiation of rollout_kernel (SPEC §10's record, §11's
// interruption, §14's value-ranked choice, §15's audit: the table in scg_rollout_kernel.hpp) and trial_kernel<true>, reached through
// launch_rollout<REC, Args> / launch_trial_record, which the two kernel headers declare.
// scg_rollout_population.hip is a unit of the same kind: SPEC §21's four population instantiations of rollout_kernel,
// reached through the same launch_rollout<REC, Args>; with SPEC §24.1's pop_clf the same four stage a classifier table per policy
// (DESIGN §3.29); SPEC §25.1's pop_gate takes a fifth one, whose value gate compares under a gate table per policy.
// scg_step_gate.hip is another: SPEC §26's step_gate_kernel (scg_step_gate_kernel.hpp: here its arguments and launch_step_gate's declaration
// only), launched by scg_step_gated between td_kernel and the reduce launch.
// scg_returns.hip holds SPEC §27's two kernels (scg_returns.hpp: here their arguments and launches only), behind scg_row_values and
// scg_lambda_returns, and SPEC §28's trace_returns_kernel behind scg_trace_returns.
// scg_returns_cross.hip holds SPEC §29's row_values_cross_kernel behind scg_row_values_cross.
// scg_record_store.hip holds SPEC §30.1's record store kernels behind scg_record_append, scg_record_offsets and scg_record_pack
// (DESIGN §3.35).
// scg_ridge.hip holds SPEC §31's pinned-order ridge solve, ridge_factor_kernel (one launch per block column of 16) and
// ridge_subst_kernel, behind scg_ridge_solve (scg_ridge.hpp: here their arguments and the launch only).
// Every sum has the pinned order of SPEC §3.1 / §5 / §6 (no atomics on data): the CPU oracle reproduces every bit.
// No upstream code exists to cite (reference = README.md:1-2); sections cite SPEC.md.
#include "scg_device.hpp"
#include "../../include/scg_abi.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <mutex>
#include <new>
#include <type_traits>
#include <vector>

using namespace scg;
typedef float f4v __attribute__((ext_vector_type(4)));
typedef unsigned u4v __attribute__((ext_vector_type(4)));

#include "scg_eval.hpp"
#include "scg_step_kernel.hpp"
#include "scg_rollout_kernel.hpp"
#include "scg_trial_kernel.hpp"
#include "scg_order.hpp"
#include "scg_collect_kernels.hpp"
#include "scg_reduce_kernel.hpp"
#include "scg_apply_kernels.hpp"
#include "scg_aux_kernels.hpp"
#include "scg_gram_kernel.hpp"
#include "scg_basis_kernels.hpp"
#include "scg_step_gate_kernel.hpp"
#include "scg_returns.hpp"
#include "scg_returns_cross.hpp"
#include "scg_record_store.hpp"
#include "scg_ridge.hpp"

// ------------------------------------------------------------------------------------------------
// host side: the C-ABI
struct scg_ctx {
    scg_config cfg;
    int n_vf;
    int nblk;
    int n_cu;                      // compute units of the device (picks the reduce launch's form)
    bool have_map;
    MapScalars ms;
    float *d_edges, *d_starts, *d_scale;
    uint64_t *d_cellmask;
    int32_t *d_perm, *d_hist;      // SPEC §5 env order of the current step (d_hist: scratch of the stand-alone sort)
    int32_t *d_collect_rows;       // scg_collect_examples: per-row totals [rows of COL_ROW envs] + the buffer's fill level
    int32_t *d_frontier_rows;      // scg_collect_frontier: the same per node [MAX_VF][rows + 1] (its own: an announced
                                   // trigger's totals in d_collect_rows survive a frontier collection)
    uint32_t arm_bits;             // scg_arm_collect: the announced trigger (0 = none) ...
    const uint8_t *arm_prev;
    const int32_t *arm_count;
    int32_t arm_L;
    bool arm_rows_ready;           // ... and whether the last scg_step left its row totals in d_collect_rows
    unsigned long long *d_fit_part;   // fit_kernel: tagged workgroup partials [FIT_BATCH][2][FIT_G][8]
    uint32_t *h_async;             // pinned, device-visible status word: kernels that give up OR their reason into it
    uint32_t *d_async;             // ... its device address
    int32_t *d_fail;               // device-side twin of the step's give-up bit (read by the reduce launch of the same step)
    double fit_timeout_s;          // how long fit_kernel waits for a workgroup that is not running yet
    float4 *d_outrec;              // [nblk * BLOCK_ENVS][OREC] per-position step results (td_kernel -> commit_row)
    float4 *d_qalt;                // [nblk * BLOCK_ENVS][2] the root's Q(s', .) of envs about to enter an option (SPEC §4.2)
    int32_t *d_invperm;            // [n_envs] position of each env in d_perm
    int32_t *d_hist2[2];           // per-row counts of the option ids a learning step leaves (double-buffered)
    int hist_parity;
    bool hist_dirty;               // a failed call may have left counts behind: clear both before the next use
    bool order_valid;              // d_perm already holds the order of the ids in order_ids (made by the last learning step)
    const int32_t *order_ids;
    uint32_t parents;              // packed option targets (default: the chain k -> k-1)
    uint32_t gest;                 // SPEC §4.4 options in gestation
    int32_t *gest_succ;            // caller-owned device counters [n_vf] (NULL = none)
    float *ring_x, *ring_y;        // SPEC §7 caller-owned trace buffers (NULL = off)
    uint8_t *events;
    int32_t *ev_len;
    int32_t ring_len;
    unsigned long long *d_stamps;   // diagnostic build only (NULL otherwise)
    float *d_slabs;
    int32_t *d_cnts;
    float *d_G;
    int32_t *d_nk;
    float *G_out;          // where reduce leaves G / n_k (ctx-owned by default)
    int32_t *nk_out;
    float *nkf_out;        // packed operand: float copy of the counts right after G (null = off)
    bool prof_on;          // measurement hook: event pairs round the fused kernel
    int prof_every;        // ... of every prof_every-th launch (events cost a few us of queue bubble each)
    long long prof_seen;
    std::vector<hipEvent_t> *prof_ev;
    size_t prof_used;
    // peer transport (scg_peer_*): this rank's region, the peers' mappings and the private exchange counter
    char *peer_region;             // hipMalloc'd: [epoch line][void line][operand parity 0][operand parity 1]
    size_t peer_bytes, peer_op_stride;        // region size; bytes from one operand to the next
    hipIpcMemHandle_t peer_handle;
    int peer_n, peer_rank;         // 0 = not opened
    char *peer_base[PEER_MAX];     // every rank's region (own or mapped)
    bool peer_mapped[PEER_MAX];    // opened with hipIpcOpenMemHandle (closed at destroy)
    uint32_t peer_e;               // exchanges done: the epoch a rank publishes is peer_e + 1
    int32_t *d_peer_go;            // peer_wait_kernel -> apply_peers_kernel: apply (1) or not (0)
    double peer_timeout_s;
    char err[256];
};

// Regions exported by this process: a peer ctx in the SAME process is found here instead of being IPC-opened (the runtime may
// refuse to open a handle of the calling process).
static std::mutex g_peer_mu;
static std::vector<std::pair<hipIpcMemHandle_t, char *>> g_peer_regions;

static thread_local char g_err[256] = "";

#define SCG_HIP(ctx, call)                                                                     \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            snprintf((ctx) ? (ctx)->err : g_err, 256, "%s failed: %s", #call, hipGetErrorString(e_)); \
            return SCG_ERR_HIP;                                                                \
        }                                                                                      \
    } while (0)

static int fail(scg_ctx *ctx, int code, const char *msg) {
    snprintf(ctx ? ctx->err : g_err, 256, "%s", msg);
    return code;
}

// an error of entry point `fn`: "fn: why"
static int fail_in(scg_ctx *c, int code, const char *fn, const char *why) {
    char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s", fn, why);
    return fail(c, code, msg);
}

static bool pow2(int x) { return x > 0 && !(x & (x - 1)); }
// an example window (SPEC §7): l_pos most recent states labelled 1, then l_neg labelled 0; at least one, the sum an int32
static bool bad_window(int32_t l_pos, int32_t l_neg) {
    return l_pos < 0 || l_neg < 0 || (int64_t)l_pos + l_neg < 1 || (int64_t)l_pos + l_neg > INT32_MAX;
}

// Sticky device-side failures (include/scg_abi.h, "asynchronous failures"): checked before every launch.
static int decode_async(uint32_t word, char *buf, size_t n) {
    if (word == 0) { if (buf && n) buf[0] = 0; return SCG_OK; }
    if (buf && n) {
        if (word & SCG_ASYNC_STEP_HANDOFF)
            snprintf(buf, n, "an earlier scg_step gave up inside a workgroup: a bounded hand-off poll between its wavefront subsets ran "
                     "out (a logic error or a hung wavefront); the block's partial gradients were dropped and the step's outputs for "
                     "its envs are unspecified — restore the state. scg_clear_async_error() re-arms the context");
        else if (word & SCG_ASYNC_PEER_TIMEOUT)
            snprintf(buf, n, "an earlier scg_peer_exchange_apply gave up: the peer wait ran out (a peer rank did not publish its "
                     "operand within the peer timeout: stopped, hung or out of step); the weights were left unchanged. "
                     "scg_clear_async_error() re-arms the context");
        else if (word & SCG_ASYNC_FIT_TIMEOUT)
            snprintf(buf, n, "an earlier scg_fit_initiation gave up (problem mask 0x%x): its workgroups did not become "
                     "co-resident within the fit timeout (card shared with other work?); the affected classifier rows were "
                     "left unchanged. scg_clear_async_error() re-arms the context", (word >> 8) & 0xffffu);
        else
            snprintf(buf, n, "unknown asynchronous device status 0x%x", word);
    }
    return SCG_ERR_ASYNC;
}
static int async_pending(scg_ctx *c);
#define SCG_CHECK_ASYNC(c) do { if (async_pending(c)) return SCG_ERR_ASYNC; } while (0)

// Every entry point that touches the device runs with the ctx's device current and leaves the caller's current
// device as it found it (a multi-GPU caller that forgot torch.cuda.set_device would otherwise launch on the
// wrong card, against buffers owned by another GPU).
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess) { ok = false; return; }
        if (cur != dev) {
            if (hipSetDevice(dev) != hipSuccess) { ok = false; return; }
            prev = cur;
        }
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};
#define SCG_ON_DEVICE(c, what)                                                                   \
    DeviceGuard dev_guard_((c)->cfg.device);                                                     \
    if (!dev_guard_.ok) return fail((c), SCG_ERR_HIP, what ": cannot make the context's device current")

static int async_pending(scg_ctx *c) {
    if (!c || !c->h_async) return 0;
    const uint32_t w = *reinterpret_cast<volatile uint32_t *>(c->h_async);
    if (w == 0) return 0;
    decode_async(w, c->err, sizeof(c->err));
    return 1;
}

extern "C" {

int scg_abi_version(void) { return SCG_ABI_VERSION; }

int scg_decode_async_word(uint32_t word, char *buf, int32_t buf_len) {
    return decode_async(word, buf, buf_len > 0 ? (size_t)buf_len : 0);
}

int scg_async_status(scg_ctx *c, void *stream, int32_t synchronize, uint32_t *word_out) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_async_status: null ctx");
    if (synchronize) {
        SCG_ON_DEVICE(c, "scg_async_status");
        SCG_HIP(c, hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    }
    const uint32_t w = c->h_async ? *reinterpret_cast<volatile uint32_t *>(c->h_async) : 0u;
    if (word_out) *word_out = w;
    return decode_async(w, c->err, sizeof(c->err));
}

int scg_clear_async_error(scg_ctx *c) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_clear_async_error: null ctx");
    if (c->h_async) *reinterpret_cast<volatile uint32_t *>(c->h_async) = 0u;
    // a step that gave up was voided on the device (no apply, no commit): whatever it left half-made is dropped here
    if (c->d_fail) {
        DeviceGuard g(c->cfg.device);
        if (g.ok) (void)hipMemset(c->d_fail, 0, sizeof(int32_t));
    }
    c->order_valid = false; c->hist_dirty = true; c->arm_rows_ready = false;
    return SCG_OK;
}

static int set_timeout(scg_ctx *c, const char *fn, double scg_ctx::*field, double seconds) {
    if (!c) return fail_in(nullptr, SCG_ERR_INVALID, fn, "null ctx");
    if (!(seconds >= 0.0) || seconds > 3600.0) return fail_in(c, SCG_ERR_INVALID, fn, "seconds must be in [0, 3600]");
    c->*field = seconds;
    return SCG_OK;
}

int scg_set_fit_timeout(scg_ctx *c, double seconds) { return set_timeout(c, "scg_set_fit_timeout", &scg_ctx::fit_timeout_s, seconds); }

int scg_set_peer_timeout(scg_ctx *c, double seconds) { return set_timeout(c, "scg_set_peer_timeout", &scg_ctx::peer_timeout_s, seconds); }

int scg_debug_raise_async(scg_ctx *c, uint32_t word) {
    if (!c || !c->h_async) return fail(c, SCG_ERR_INVALID, "scg_debug_raise_async: null ctx");
    *reinterpret_cast<volatile uint32_t *>(c->h_async) |= word;
    return SCG_OK;
}

int scg_block_envs(void) { return BLOCK_ENVS; }

const char *scg_strerror(int status) {
    switch (status) {
        case SCG_OK: return "ok";
        case SCG_ERR_INVALID: return "invalid argument";
        case SCG_ERR_NO_DEVICE: return "no usable HIP device";
        case SCG_ERR_HIP: return "HIP runtime error";
        case SCG_ERR_STATE: return "call order / state error";
        case SCG_ERR_ASYNC: return "an earlier launch failed on the device";
        default: return "unknown status";
    }
}

const char *scg_last_error(const scg_ctx *ctx) { return ctx ? ctx->err : g_err; }

static size_t hist_bytes(const scg_ctx *c) { return (size_t)((c->cfg.n_envs + 255) / 256) * HSTRIDE * sizeof(int32_t); }

// The context's device allocations of fixed size: scg_create walks the table to allocate (and clear), scg_destroy to free.
// (Not here: d_starts, sized by scg_set_map; the pinned h_async; the peer region; the event pool.)
struct CtxAlloc { void **ptr; size_t bytes; bool zero; };
static std::vector<CtxAlloc> ctx_allocs(scg_ctx *c) {
    auto P = [](auto **p) { return reinterpret_cast<void **>(p); };
    const size_t w = (size_t)c->n_vf * NACT * NF * sizeof(float), npos = (size_t)c->nblk * BLOCK_ENVS;
    const size_t rows = (size_t)(c->cfg.n_envs + COL_ROW - 1) / COL_ROW + 1;
    return {
        {P(&c->d_slabs), (size_t)c->nblk * w, false},
        {P(&c->d_cnts), (size_t)c->nblk * c->n_vf * sizeof(int32_t), true},
        {P(&c->d_G), w, true},
        {P(&c->d_nk), MAX_VF * sizeof(int32_t), true},
        {P(&c->d_edges), MAX_EDGES * 8 * sizeof(float), false},
        {P(&c->d_scale), NF * sizeof(float), false},
        {P(&c->d_perm), npos * sizeof(int32_t), false},
        {P(&c->d_hist), hist_bytes(c), false},
        {P(&c->d_collect_rows), rows * sizeof(int32_t), false},
        {P(&c->d_frontier_rows), MAX_VF * rows * sizeof(int32_t), false},
        {P(&c->d_fit_part), (size_t)FIT_BATCH * 2 * FIT_G * 8 * sizeof(unsigned long long), false},
        {P(&c->d_fail), sizeof(int32_t), true},
        {P(&c->d_outrec), npos * OREC * sizeof(float4), false},
        {P(&c->d_qalt), npos * 2 * sizeof(float4), false},
        {P(&c->d_invperm), npos * sizeof(int32_t), false},
        {P(&c->d_hist2[0]), hist_bytes(c), true},
        {P(&c->d_hist2[1]), hist_bytes(c), true},
        {P(&c->d_cellmask), (size_t)CELL_G * CELL_G * 4 * sizeof(uint64_t), false},
    };
}

#ifdef SCG_REDUCE_STAMPS
static size_t reduce_stamp_bytes(const scg_ctx *c) {      // the largest reduce grid of this context: the slab workgroups + one slot per row of 256 envs
    const int nrow = (c->cfg.n_envs + 255) / 256, sy = (nrow + RED_NCOL - 1) / RED_NCOL;
    return (size_t)RED_NCOL * (c->n_vf + sy) * RED_STAMP_SLOTS * sizeof(unsigned long long);
}
#endif

int scg_create(scg_ctx **out, const scg_config *cfg) {
    if (!out || !cfg) return fail(nullptr, SCG_ERR_INVALID, "scg_create: null argument");
    *out = nullptr;
    if (cfg->n_envs < 1) return fail(nullptr, SCG_ERR_INVALID, "scg_create: n_envs must be >= 1");
    if (cfg->n_options < 0 || cfg->n_options > SCG_MAX_OPTIONS)
        return fail(nullptr, SCG_ERR_INVALID, "scg_create: n_options out of range [0,5]");
    if (cfg->update_count_floor < 0) return fail(nullptr, SCG_ERR_INVALID, "scg_create: update_count_floor must be >= 0");
    if (cfg->reoffer_period != 0 && !pow2(cfg->reoffer_period))
        return fail(nullptr, SCG_ERR_INVALID, "scg_create: reoffer_period must be a power of two (or 0)");
    if (cfg->fourier_order != SCG_FOURIER_ORDER)
        return fail(nullptr, SCG_ERR_INVALID, "scg_create: only Fourier order 5 is built");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(nullptr, SCG_ERR_NO_DEVICE, "scg_create: no HIP device visible");
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(nullptr, SCG_ERR_INVALID, "scg_create: device ordinal out of range");
    scg_ctx *c = new (std::nothrow) scg_ctx();
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_create: out of host memory");
    memset(c, 0, sizeof(*c));
    c->cfg = *cfg;
    c->n_vf = cfg->n_options + 1;
    c->nblk = (cfg->n_envs + BLOCK_ENVS - 1) / BLOCK_ENVS;
    if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, cfg->device) != hipSuccess || c->n_cu <= 0) c->n_cu = 256;
    int st = SCG_OK;
    DeviceGuard dev_guard_(cfg->device);
    do {
        if (!dev_guard_.ok) { st = SCG_ERR_HIP; break; }
        for (const CtxAlloc &a : ctx_allocs(c)) {
            if (hipMalloc(a.ptr, a.bytes) != hipSuccess || (a.zero && hipMemset(*a.ptr, 0, a.bytes) != hipSuccess)) { st = SCG_ERR_HIP; break; }
        }
        if (st != SCG_OK) break;
        if (hipHostMalloc(reinterpret_cast<void **>(&c->h_async), 64, hipHostMallocMapped) != hipSuccess) { st = SCG_ERR_HIP; break; }
        *c->h_async = 0u;
        if (hipHostGetDevicePointer(reinterpret_cast<void **>(&c->d_async), c->h_async, 0) != hipSuccess) { st = SCG_ERR_HIP; break; }
        // (the step kernel's LDS — 160 KB, one workgroup per CU — is static: no dynamic-LDS attribute to raise)
    } while (0);
    if (st != SCG_OK) {
        snprintf(g_err, 256, "scg_create: device allocation/setup failed: %s", hipGetErrorString(hipGetLastError()));
        scg_destroy(c);
        return st;
    }
#ifdef SCG_STAMPS_LITE
    if (hipMalloc(&c->d_stamps, (size_t)c->nblk * STAMP_SLOTS * sizeof(unsigned long long)) == hipSuccess)
        (void)hipMemset(c->d_stamps, 0, (size_t)c->nblk * STAMP_SLOTS * sizeof(unsigned long long));
#endif
#ifdef SCG_REDUCE_STAMPS
    if (hipMalloc(&c->d_stamps, reduce_stamp_bytes(c)) == hipSuccess) (void)hipMemset(c->d_stamps, 0, reduce_stamp_bytes(c));
#endif
    c->parents = 0;
    for (int k = 1; k < MAX_VF; ++k) c->parents |= (uint32_t)(k - 1) << (3 * k);      // chain: 1 -> goal, k -> k-1
    c->G_out = c->d_G; c->nk_out = c->d_nk;
    c->fit_timeout_s = 2.0;
    c->peer_timeout_s = 2.0;
    *out = c;
    return SCG_OK;
}

int scg_destroy(scg_ctx *c) {
    if (!c) return SCG_OK;
    for (const CtxAlloc &a : ctx_allocs(c)) (void)hipFree(*a.ptr);
    (void)hipFree(c->d_starts);
    if (c->h_async) (void)hipHostFree(c->h_async);
    if (c->peer_region) {
        DeviceGuard g(c->cfg.device);
        for (int r = 0; r < PEER_MAX; ++r)
            if (c->peer_mapped[r]) (void)hipIpcCloseMemHandle(c->peer_base[r]);
        {
            std::lock_guard<std::mutex> lk(g_peer_mu);
            for (size_t i = 0; i < g_peer_regions.size(); ++i)
                if (g_peer_regions[i].second == c->peer_region) { g_peer_regions.erase(g_peer_regions.begin() + i); break; }
        }
        (void)hipFree(c->peer_region); (void)hipFree(c->d_peer_go);
    }
    if (c->prof_ev) {
        for (hipEvent_t e : *c->prof_ev) (void)hipEventDestroy(e);
        delete c->prof_ev;
    }
    delete c;
    return SCG_OK;
}

int scg_set_hparams(scg_ctx *c, float gamma, float alpha, float epsilon, float r_option_success,
                    int32_t max_episode_steps, int32_t max_option_steps, int32_t update_count_floor, int32_t reoffer_period) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_set_hparams: null ctx");
    // validate first: a refused call changes nothing (the same two checks as scg_create)
    if (update_count_floor < 0) return fail(c, SCG_ERR_INVALID, "scg_set_hparams: update_count_floor must be >= 0");
    if (reoffer_period != 0 && !pow2(reoffer_period)) return fail(c, SCG_ERR_INVALID, "scg_set_hparams: reoffer_period must be a power of two (or 0)");
    c->cfg.gamma = gamma; c->cfg.alpha = alpha; c->cfg.epsilon = epsilon;
    c->cfg.r_option_success = r_option_success;
    c->cfg.max_episode_steps = max_episode_steps; c->cfg.max_option_steps = max_option_steps;
    c->cfg.update_count_floor = update_count_floor;
    c->cfg.reoffer_period = reoffer_period;
    return SCG_OK;
}

int scg_set_map(scg_ctx *c, const float *edges, int32_t n_edges, const float *starts, int32_t n_starts,
                const float map_scalars[6], const float *scale) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_set_map: null ctx");
    if (!edges || !starts || !map_scalars || !scale) return fail(c, SCG_ERR_INVALID, "scg_set_map: null argument");
    if (n_edges < 0 || n_edges > MAX_EDGES) return fail(c, SCG_ERR_INVALID, "scg_set_map: n_edges out of range [0,256]");
    if (n_starts < 1) return fail(c, SCG_ERR_INVALID, "scg_set_map: need at least one start position");
    SCG_ON_DEVICE(c, "scg_set_map");
    if (c->d_starts) { (void)hipFree(c->d_starts); c->d_starts = nullptr; }
    SCG_HIP(c, hipMalloc(&c->d_starts, (size_t)n_starts * 2 * sizeof(float)));
    if (n_edges > 0) SCG_HIP(c, hipMemcpy(c->d_edges, edges, (size_t)n_edges * 8 * sizeof(float), hipMemcpyHostToDevice));
    SCG_HIP(c, hipMemcpy(c->d_starts, starts, (size_t)n_starts * 2 * sizeof(float), hipMemcpyHostToDevice));
    SCG_HIP(c, hipMemcpy(c->d_scale, scale, NF * sizeof(float), hipMemcpyHostToDevice));
    const float R = map_scalars[0];
    c->ms.hstep = map_scalars[1]; c->ms.R2 = map_scalars[2];
    c->ms.TX = map_scalars[3]; c->ms.TY = map_scalars[4]; c->ms.TR2 = map_scalars[5];
    c->ms.R = R; c->ms.TR = (float)(std::sqrt((double)map_scalars[5]) * 1.0001);
    // Candidate masks (an internal acceleration table, not part of the arithmetic contract): cell (cx,cy)
    // lists every edge within  R(1.02 + 1.10*|v|max) + half a cell diagonal  of the cell centre, so the
    // mask of the ball's cell is a superset of the edges the per-step bound of pinball_step() can admit.
    {
        std::vector<uint64_t> cm((size_t)CELL_G * CELL_G * 4, 0);
        const double vmax = 2.0 * std::sqrt(2.0) * 1.001;
        const double reach = (double)R * (1.02 + 1.10 * vmax) * 1.01 + 0.5 * std::sqrt(2.0) / CELL_G + 1e-6;
        for (int cy = 0; cy < CELL_G; ++cy)
            for (int cx = 0; cx < CELL_G; ++cx) {
                const double px = (cx + 0.5) / CELL_G, py = (cy + 0.5) / CELL_G;
                for (int j = 0; j < n_edges; ++j) {
                    const float *E = edges + 8 * j;
                    const double dx = px - E[0], dy = py - E[1];
                    double t = (dx * E[2] + dy * E[3]) * E[4];
                    t = t < 0 ? 0 : (t > 1 ? 1 : t);
                    const double qx = E[0] + E[2] * t - px, qy = E[1] + E[3] * t - py;
                    if (std::sqrt(qx * qx + qy * qy) <= reach)
                        cm[((size_t)cy * CELL_G + cx) * 4 + (j >> 6)] |= (1ull << (j & 63));
                }
            }
        SCG_HIP(c, hipMemcpy(c->d_cellmask, cm.data(), cm.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    c->ms.n_edges = n_edges; c->ms.n_starts = n_starts;
    c->have_map = true;
    return SCG_OK;
}

// While a peer region is open, a learning step leaves its packed operand in the region's buffer of parity peer_e & 1.
struct PeerTarget {
    scg_ctx *c;
    float *G, *nkf;
    int32_t *nk;
    explicit PeerTarget(scg_ctx *ctx) : c(ctx), G(ctx->G_out), nkf(ctx->nkf_out), nk(ctx->nk_out) {
        if (!c->peer_n) return;
        float *op = reinterpret_cast<float *>(c->peer_region + PEER_HDR + (c->peer_e & 1u) * c->peer_op_stride);
        c->G_out = op; c->nkf_out = op + (size_t)c->n_vf * NACT * NF; c->nk_out = c->d_nk;
    }
    ~PeerTarget() { c->G_out = G; c->nkf_out = nkf; c->nk_out = nk; }
};

// the per-context parameters of the step and the rollout kernel (StepArgs, RolloutArgs); every other field zero
extern "C++" template <typename Args>
static void fill_shared(const scg_ctx *c, Args &A) {
    memset(&A, 0, sizeof(A));
    A.n = c->cfg.n_envs; A.n_vf = c->n_vf;
    A.seed = c->cfg.seed; A.env_base = c->cfg.env_id_base;
    A.epsilon = c->cfg.epsilon; A.max_ep = c->cfg.max_episode_steps; A.max_opt = c->cfg.max_option_steps;
    A.reoffer_mask = c->cfg.reoffer_period > 1 ? (uint32_t)(c->cfg.reoffer_period - 1) : 0u;
    A.parents = c->parents; A.gest = c->gest;
    A.ms = c->ms;
    A.edges = c->d_edges; A.starts = c->d_starts; A.cellmask = c->d_cellmask;
}

static void fill_common(const scg_ctx *c, StepArgs &A) {
    fill_shared(c, A);
    A.gamma = c->cfg.gamma; A.r_succ = c->cfg.r_option_success;
    A.slabs = c->d_slabs; A.cnts = c->d_cnts;
    A.gest_succ = c->gest_succ;
    A.ring_x = c->ring_x; A.ring_y = c->ring_y; A.events = c->events; A.ev_len = c->ev_len;
    A.ring_mask = c->ring_len > 0 ? c->ring_len - 1 : 0;
    A.stamps = c->d_stamps;
    A.async_word = c->d_async; A.fail_flag = c->d_fail;
}

// The reduce launch. For the fused step (every mode but REDUCE_ONLY, with the step's arguments `st`) extra workgroups commit the
// step's per-position results to the caller's arrays and, in the last mode, place every row in the next step's env order; an
// acting-only step has nothing to reduce and launches the commit alone.
enum ReduceMode { REDUCE_ONLY, COMMIT_ONLY, REDUCE_COMMIT, REDUCE_COMMIT_SORT };
static int launch_reduce(scg_ctx *c, float *W, uint32_t apply, int nblk, hipStream_t s, ReduceMode mode, const StepArgs *st = nullptr) {
    ReduceArgs R;
    memset(&R, 0, sizeof(R));
    R.slabs = c->d_slabs; R.cnts = c->d_cnts; R.G = c->G_out; R.n_k = c->nk_out; R.nk_f = c->nkf_out; R.W = W; R.scale = c->d_scale;
    R.nblk = nblk; R.n_vf = c->n_vf; R.alpha = c->cfg.alpha; R.apply = apply; R.fail_flag = c->d_fail; R.nk_floor = c->cfg.update_count_floor;
    const int nrow = st ? (c->cfg.n_envs + 255) / 256 : 0;
    R.n = c->cfg.n_envs; R.nrow = nrow;
    if (st) {
        R.outrec = c->d_outrec; R.qalt = c->d_qalt; R.invperm = c->d_invperm; R.perm = c->d_perm; R.sort = mode == REDUCE_COMMIT_SORT ? 1 : 0;
        R.hist = c->d_hist2[c->hist_parity]; R.hist_zero = c->d_hist2[c->hist_parity ^ 1];
        R.x = st->x; R.y = st->y; R.vx = st->vx; R.vy = st->vy; R.reward = st->reward;
        R.option_id_out = st->option_id; R.opt_steps = st->opt_steps; R.ep_steps = st->ep_steps;
        R.action = st->action; R.done = st->done;
        R.qcache = st->k_hi >= 0 ? st->qcache : nullptr;
        if (c->arm_bits && c->events && c->ring_x) {
            R.c_events = c->events; R.c_prev = c->arm_prev; R.c_evlen = c->ev_len; R.c_count = c->arm_count;
            R.c_rows = c->d_collect_rows; R.c_bits = c->arm_bits; R.c_L = c->arm_L; R.c_ring_len = c->ring_len;
        }
    }
#ifdef SCG_REDUCE_STAMPS
    R.stamps = c->d_stamps;
#endif
    if (mode == COMMIT_ONLY) {
        hipLaunchKernelGGL(commit_kernel, dim3(nrow), dim3(256), 0, s, R);
        SCG_HIP(c, hipGetLastError());
        return SCG_OK;
    }
    const int sy = (nrow + RED_NCOL - 1) / RED_NCOL;            // row slots: whole lines of the grid in front of the slab workgroups' n_vf lines
    constexpr int W64 = (RED_COLS + 63) / 64;                   // the launch's size in units of 64 columns x 16 waves (+ its rows in lines of as many)
    if (W64 * (c->n_vf + (nrow + W64 - 1) / W64) <= c->n_cu)    // a small launch (at most one such unit per CU): all sixteen slabs of a segment in flight
        hipLaunchKernelGGL(reduce_kernel<16>, dim3(RED_NCOL, c->n_vf + sy), dim3(RED_THREADS), 0, s, R);
    else                                                        // 64 VGPRs: eight waves per SIMD (round 18: with all of the bench size's workgroups resident either way, this form was 0.2 % ahead there)
        hipLaunchKernelGGL(reduce_kernel<8>, dim3(RED_NCOL, c->n_vf + sy), dim3(RED_THREADS), 0, s, R);
    SCG_HIP(c, hipGetLastError());
    return SCG_OK;
}

// env order of a step (SPEC §5): counting sort by the option ids the previous step left.
// A learning step computes the NEXT step's order inside its reduce launches; the stand-alone sort runs only
// when that order is missing or was invalidated (first step, other array, scg_invalidate_order).
static int sort_env_order(scg_ctx *c, const int32_t *option_id, hipStream_t s) {
    if (c->order_valid && c->order_ids == option_id) return SCG_OK;
    const int nrow = (c->cfg.n_envs + 255) / 256;    // the sort works on rows of 256 envs whatever the workgroup size
    hipLaunchKernelGGL(sort_hist_kernel, dim3(nrow), dim3(256), 0, s, option_id, c->cfg.n_envs, c->n_vf, c->d_hist);
    hipLaunchKernelGGL(sort_scatter_kernel, dim3(nrow), dim3(256), 0, s, option_id, c->cfg.n_envs, c->n_vf, nrow,
                       c->d_hist, c->d_perm, c->d_invperm);
    SCG_HIP(c, hipGetLastError());
    return SCG_OK;
}

// measurement hook: on a sampled launch, record the first event of a pair and hand back the second (else ev1 stays null)
static int prof_begin(scg_ctx *c, hipStream_t s, hipEvent_t &ev1) {
    if (!(c->prof_on && (c->prof_seen++ % c->prof_every) == c->prof_every / 2)) return SCG_OK;     // (not the first launch into an idle queue)
    if (!c->prof_ev) c->prof_ev = new std::vector<hipEvent_t>();
    while (c->prof_ev->size() < c->prof_used + 2) {
        hipEvent_t e;
        SCG_HIP(c, hipEventCreate(&e));
        c->prof_ev->push_back(e);
    }
    hipEvent_t ev0 = (*c->prof_ev)[c->prof_used];
    ev1 = (*c->prof_ev)[c->prof_used + 1];
    c->prof_used += 2;
    SCG_HIP(c, hipEventRecord(ev0, s));
    return SCG_OK;
}

int scg_step(scg_ctx *c, float *x, float *y, float *vx, float *vy, int32_t *option_id, int32_t *opt_steps,
             int32_t *ep_steps, float *qcache, uint8_t *action, float *reward, uint8_t *done, float *W,
             const float *clf, uint32_t enabled_mask, uint64_t t, uint32_t flags, void *stream) {
    return scg_step_gated(c, x, y, vx, vy, option_id, opt_steps, ep_steps, qcache, action, reward, done, W, clf, enabled_mask, t, flags,
                          stream, nullptr, 0u);
}

// positions per workgroup of a step_gate_kernel launch: the largest of 64, 128, 256 that still gives every CU a workgroup (DESIGN
// §3.31: a short range at small env counts, where the launch is latency, full units at large ones); the results do not depend on it.
// SCG_STEP_GATE_ENVS (64, 128 or 256) pins it instead: a hook for tests and measurements, as SCG_ROLLOUT_EPW. false: another value
static bool step_gate_envs(const scg_ctx *c, int &envs) {
    envs = SG_MIN_ENVS;
    while (envs < SG_MAX_ENVS && (long long)c->cfg.n_envs >= (long long)c->n_cu * envs * 2) envs *= 2;
    if (const char *ov = getenv("SCG_STEP_GATE_ENVS")) {
        const int v = atoi(ov);
        if (v != 64 && v != 128 && v != 256) return false;
        envs = v;
    }
    return true;
}

// SPEC §26.1: scg_step whose entry decisions of the options in gate_mask compare under a gate table. gate_mask == 0 is scg_step, launch
// for launch; otherwise step_gate_kernel runs between td_kernel and the reduce launch (also in front of an acting-only step's commit
// launch) and re-decides the entering envs from what td_kernel left in their result lines.
int scg_step_gated(scg_ctx *c, float *x, float *y, float *vx, float *vy, int32_t *option_id, int32_t *opt_steps,
                   int32_t *ep_steps, float *qcache, uint8_t *action, float *reward, uint8_t *done, float *W,
                   const float *clf, uint32_t enabled_mask, uint64_t t, uint32_t flags, void *stream,
                   const float *gate, uint32_t gate_mask) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_step: null ctx");
    if (!c->have_map) return fail(c, SCG_ERR_STATE, "scg_step: scg_set_map has not been called");
    if (!x || !y || !vx || !vy || !option_id || !opt_steps || !ep_steps || !qcache || !action || !reward ||
        !done || !W || !clf)
        return fail(c, SCG_ERR_INVALID, "scg_step: null array argument");
    if (c->peer_n && (flags & SCG_STEP_LEARN) && (flags & SCG_STEP_APPLY))
        return fail(c, SCG_ERR_INVALID, "scg_step: SCG_STEP_APPLY with a peer region open (the update is scg_peer_exchange_apply's)");
    if ((flags & SCG_STEP_INTERRUPT) && !(flags & SCG_STEP_LEARN))
        return fail(c, SCG_ERR_INVALID, "scg_step: SCG_STEP_INTERRUPT without SCG_STEP_LEARN (acting-only interruption is scg_rollout_interrupt)");
    SCG_CHECK_ASYNC(c);
    SCG_ON_DEVICE(c, "scg_step");
    if (c->arm_bits) {
        // An announced trigger (scg_arm_collect) makes this step's commit rows read the caller's prev_in / count buffers:
        // refuse to launch if they are no longer device allocations (freed since the announcement) instead of faulting
        // the GPU. Two host-side attribute queries per step, only while a trigger is armed.
        const void *ptrs[2] = {c->arm_count, c->arm_prev};
        for (const void *p : ptrs) {
            if (!p) continue;
            hipPointerAttribute_t at;
            if (hipPointerGetAttributes(&at, p) != hipSuccess || at.type != hipMemoryTypeDevice) {
                (void)hipGetLastError();
                c->arm_bits = 0; c->arm_rows_ready = false;
                return fail(c, SCG_ERR_STATE, "scg_step: the buffers announced with scg_arm_collect are no longer device memory "
                                              "(freed before scg_arm_collect(0)?); the trigger has been disarmed");
            }
        }
    }
    int gate_envs = 0;
    if (gate_mask) {                                // SPEC §26.1's refusals, behind scg_step's own and in this order
        if (!gate) return fail(c, SCG_ERR_INVALID, "scg_step_gated: gate_mask without a gate table");
        if ((gate_mask & 1u) || (c->n_vf < 32 && (gate_mask >> c->n_vf)))
            return fail(c, SCG_ERR_INVALID, "scg_step_gated: gate_mask names the root (bit 0) or an option the context does not have");
        if (flags & SCG_STEP_INTERRUPT)
            return fail(c, SCG_ERR_INVALID, "scg_step_gated: gate_mask with SCG_STEP_INTERRUPT (a gated interrupting learner is not defined)");
        if (flags & 0x100u) return fail(c, SCG_ERR_INVALID, "scg_step_gated: gate_mask with the diagnostic flag 0x100 (no values to commit)");
        if (!step_gate_envs(c, gate_envs)) return fail(c, SCG_ERR_INVALID, "scg_step_gated: SCG_STEP_GATE_ENVS must be 64, 128 or 256");
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    StepArgs A;
    fill_common(c, A);
    A.x = x; A.y = y; A.vx = vx; A.vy = vy;
    A.option_id = option_id; A.opt_steps = opt_steps; A.ep_steps = ep_steps; A.qcache = qcache;
    A.action = action; A.reward = reward; A.done = done;
    A.W = W; A.clf = clf;
    A.k_lo = 0; A.k_hi = c->n_vf - 1;
    A.enabled = enabled_mask; A.learn = (flags & SCG_STEP_LEARN) ? 1u : 0u; A.t = t;
    if (flags & 0x100u) A.k_hi = -1;     // diagnostic only (bench.py --diag-no-td): skip the TD passes
    if (const int rc = sort_env_order(c, option_id, s)) return rc;
    c->order_valid = false;
    if (c->hist_dirty) {
        const size_t hb = hist_bytes(c);
        SCG_HIP(c, hipMemsetAsync(c->d_hist2[0], 0, hb, s));
        SCG_HIP(c, hipMemsetAsync(c->d_hist2[1], 0, hb, s));
        c->hist_dirty = false;
    }
    const bool fold = (flags & SCG_STEP_LEARN) && !(flags & 0x200u);      // 0x200: diagnostic, sort afresh every step
    A.hist_next = fold ? c->d_hist2[c->hist_parity] : nullptr;
    A.perm = c->d_perm; A.outrec = c->d_outrec; A.qalt = c->d_qalt;
    hipEvent_t ev1 = nullptr;
    if (const int rc = prof_begin(c, s, ev1)) return rc;
    if (flags & SCG_STEP_INTERRUPT)                 // SPEC §12: the interrupting learner (only the targets and results of interrupted envs differ)
        hipLaunchKernelGGL(td_kernel<MODE_FUSED_INT>, dim3(c->nblk), dim3(THREADS), 0, s, A);
    else
        hipLaunchKernelGGL(td_kernel<MODE_FUSED>, dim3(c->nblk), dim3(THREADS), 0, s, A);
    SCG_HIP(c, hipGetLastError());
    if (gate_mask) {                                // SPEC §26.1: the masked options' entering envs are re-decided under the table
        StepGateArgs GA;
        memset(&GA, 0, sizeof(GA));
        GA.outrec = c->d_outrec; GA.perm = c->d_perm; GA.hist_next = A.hist_next; GA.gate = gate; GA.fail_flag = c->d_fail;
        GA.n = c->cfg.n_envs; GA.n_vf = c->n_vf; GA.mask = gate_mask;
        SCG_HIP(c, launch_step_gate(GA, gate_envs, s));
    }
    if (ev1) SCG_HIP(c, hipEventRecord(ev1, s));
    // results reach the caller's arrays through the commit workgroups of the reduce launch (or a commit launch)
    c->arm_rows_ready = c->arm_bits && c->events && c->ring_x;      // ... which also leave an announced trigger's row totals
    if (!(flags & SCG_STEP_LEARN)) return launch_reduce(c, W, 0u, c->nblk, s, COMMIT_ONLY, &A);
    // peer transport: the packed operand goes to this rank's buffer of the next exchange's parity (scg_peer_step_begin folded in)
    PeerTarget peer_target(c);
    if (!fold) return launch_reduce(c, W, (flags & SCG_STEP_APPLY) ? 1u : 0u, c->nblk, s, REDUCE_COMMIT, &A);
    c->hist_dirty = true;                          // until the reduce launch has consumed and re-armed the counts
    const int rc = launch_reduce(c, W, (flags & SCG_STEP_APPLY) ? 1u : 0u, c->nblk, s, REDUCE_COMMIT_SORT, &A);
    if (rc != SCG_OK) return rc;
    c->hist_dirty = false;
    c->hist_parity ^= 1;
    c->order_valid = true; c->order_ids = option_id;
    return SCG_OK;
}

// envs per wave of a rollout_kernel / trial_kernel launch over n items: the largest of 2 .. 32 that still gives every CU a
// workgroup (one 8-wave workgroup per CU: LDS); the results do not depend on it. SCG_ROLLOUT_EPW (2, 4, 8, 16 or 32) pins the
// launch geometry instead: a hook for tests and measurements, which run every geometry at any count (the results are the same
// by construction; the tests check that they are). false: SCG_ROLLOUT_EPW holds another value
static bool rollout_epw(const scg_ctx *c, int n, int &epw) {
    epw = 2;
    while (epw < RO_MAX_EPW && (long long)n >= (long long)c->n_cu * RO_WAVES * epw * 2) epw *= 2;
    if (const char *ov = getenv("SCG_ROLLOUT_EPW")) {
        const int v = atoi(ov);
        if (v < 2 || v > RO_MAX_EPW || !pow2(v)) return false;
        epw = v;
    }
    return true;
}

// a record's window and rows against N items and at least min_rows rows (SPEC §10)
static int check_record(scg_ctx *c, const char *fn, const scg_record *rec, int N, long long min_rows) {
    const char *why = !rec->len ? "rec->len is required" : rec->n < 1 ? "rec->n must be >= 1"
                    : rec->first < 0 || (long long)rec->first + rec->n > N ? "rec->first .. first+n-1 outside the envs / entries"
                    : rec->rows < min_rows ? "rec->rows too small for the launch's pseudo-steps" : nullptr;
    return why ? fail_in(c, SCG_ERR_INVALID, fn, why) : SCG_OK;
}

// a derived argument struct (record, interrupt, ...): its base (the launch's plain arguments), every member of its own zero
extern "C++" template <typename Derived, typename Base>
static Derived derived_args(const Base &base) {
    Derived D;
    memset(&D, 0, sizeof(D));
    static_cast<Base &>(D) = base;
    return D;
}

// one call of a rollout entry point: each of the five fills in what it takes, the members behind `stream` stay null / zero otherwise
struct RolloutCall {
    float *x, *y, *vx, *vy;
    int32_t *option_id, *opt_steps, *ep_steps;
    float *qcache;
    uint8_t *action;
    float *reward;
    uint8_t *done;
    const float *W, *clf;
    uint32_t enabled_mask;
    uint64_t t0;
    int32_t n_steps;
    uint32_t flags;
    const scg_rollout_stats *stats;
    void *stream;
    bool takes_begin_at;           // every entry point but scg_rollout knows SCG_ROLLOUT_BEGIN_AT
    const scg_record *rec;
    int32_t *interrupts, *overrides;
    uint32_t rules;                // SCG_SELECT_*; scg_rollout_interrupt: SCG_SELECT_INTERRUPT
    const scg_audit *audit;
    const uint8_t *first_action;   // scg_rollout_branch (SPEC §19)
    const scg_population *pop;     // scg_rollout_population (SPEC §21)
    const float *pop_clf;          // scg_rollout_population_clf (SPEC §24.1): [C][n_vf][8], a classifier table per policy
    const float *pop_gate;         // scg_rollout_population_gate (SPEC §25.1): [C][n_vf][2][5][1296], a gate table per policy
};

// the nine rollout entry points (`fn` names the caller in error texts). The kernel follows from what the call asks for:
//   audit      a member of `audit` given (SPEC §15; every member NULL counts as no audit), or a first_action (SPEC §19: the AUDIT
//              kernels are the ones that read it; with no audit member they write nothing of the audit's)
//   best, intr SCG_SELECT_BEST / SCG_SELECT_INTERRUPT in `rules` (SPEC §14 / §11), counting into `overrides` / `interrupts`
//   rec, at    a record (SPEC §10) / SCG_ROLLOUT_BEGIN_AT, from here on BEGIN in `flags` plus `at`
//   pop        a population (SPEC §21): a RolloutPop by (intr, best), whatever else the call asks for (they are AUDIT kernels, and with
//              no audit member and no first_action they write nothing of either), on a grid of whole workgroups per policy
//   pop_clf    a classifier table per policy (SPEC §24.1): the same RolloutPop kernels, which then stage pop_clf[c] where they staged
//              `clf`; refused without pop, behind every other refusal
//   pop_gate   a gate table per policy (SPEC §25.1): RolloutPopGateArgs' kernel, the fifth POP one; refused without pop and with
//              intr or best, behind pop_clf's refusal
// Neither audit, best, rec, at nor pop: the plain kernel, or with intr the non-recording interrupting one; otherwise a RolloutVar by
// (intr, best, audit)
static int rollout_launch(const char *fn, scg_ctx *c, RolloutCall a) {
    if (!c) return fail_in(nullptr, SCG_ERR_INVALID, fn, "null ctx");
    if (a.rules & ~(SCG_SELECT_INTERRUPT | SCG_SELECT_BEST)) return fail_in(c, SCG_ERR_INVALID, fn, "unknown rule");
    const bool intr = (a.rules & SCG_SELECT_INTERRUPT) != 0, best = (a.rules & SCG_SELECT_BEST) != 0;
    const scg_audit *audit = a.audit;
    if (audit && !audit->force && !audit->applied && !audit->cand && !audit->v_root && !audit->v_cand && !audit->disc_ret &&
        !audit->disc_g && !audit->disc_final)
        audit = nullptr;
    uint32_t flags = a.flags;
    const bool at = a.takes_begin_at && (flags & SCG_ROLLOUT_BEGIN_AT);
    if (at && (flags & SCG_ROLLOUT_BEGIN)) return fail_in(c, SCG_ERR_INVALID, fn, "SCG_ROLLOUT_BEGIN and SCG_ROLLOUT_BEGIN_AT together");
    if (at) flags = (flags & ~SCG_ROLLOUT_BEGIN_AT) | SCG_ROLLOUT_BEGIN;
    if (!c->have_map) return fail_in(c, SCG_ERR_STATE, fn, "scg_set_map has not been called");
    if (!a.x || !a.y || !a.vx || !a.vy || !a.option_id || !a.opt_steps || !a.ep_steps || !a.qcache || !a.action || !a.reward ||
        !a.done || !a.W || !a.clf)
        return fail_in(c, SCG_ERR_INVALID, fn, "null array argument");
    if (flags & ~(SCG_ROLLOUT_BEGIN | SCG_ROLLOUT_ONE_EPISODE)) return fail_in(c, SCG_ERR_INVALID, fn, "unknown flag");
    if (a.n_steps < 0 || a.n_steps > SCG_ROLLOUT_MAX_STEPS)
        return fail_in(c, SCG_ERR_INVALID, fn, "n_steps out of range [0, SCG_ROLLOUT_MAX_STEPS]");
    if (a.n_steps == 0 && !(flags & SCG_ROLLOUT_BEGIN))
        return fail_in(c, SCG_ERR_INVALID, fn, "n_steps == 0 without SCG_ROLLOUT_BEGIN (or _BEGIN_AT)");
    if ((flags & SCG_ROLLOUT_ONE_EPISODE) && !(a.stats && a.stats->finished))
        return fail_in(c, SCG_ERR_INVALID, fn, "SCG_ROLLOUT_ONE_EPISODE needs stats->finished");
    if (a.rec) {
        const int rc = check_record(c, fn, a.rec, c->cfg.n_envs, (long long)a.n_steps + ((flags & SCG_ROLLOUT_BEGIN) ? 1 : 0));
        if (rc != SCG_OK) return rc;
    }
    if (audit && audit->force && !(flags & SCG_ROLLOUT_BEGIN))
        return fail_in(c, SCG_ERR_INVALID, fn, "audit->force without SCG_ROLLOUT_BEGIN or _BEGIN_AT");
    if (audit && !audit->disc_ret != !audit->disc_g)
        return fail_in(c, SCG_ERR_INVALID, fn, "audit->disc_ret and audit->disc_g go together");
    if (a.first_action && a.n_steps == 0) return fail_in(c, SCG_ERR_INVALID, fn, "first_action with n_steps == 0: no real step to force");
    if (a.pop) {
        if (a.pop->n_policies < 1 || a.pop->n_policies > SCG_POP_MAX)
            return fail_in(c, SCG_ERR_INVALID, fn, "pop->n_policies out of range [1, SCG_POP_MAX]");
        if (a.pop->n_per < 1) return fail_in(c, SCG_ERR_INVALID, fn, "pop->n_per must be >= 1");
        if ((long long)a.pop->n_policies * (long long)a.pop->n_per != (long long)c->cfg.n_envs)
            return fail_in(c, SCG_ERR_INVALID, fn, "pop->n_policies * pop->n_per is not the context's n_envs");
    }
    SCG_CHECK_ASYNC(c);
    DeviceGuard dev_guard_(c->cfg.device);
    if (!dev_guard_.ok) return fail_in(c, SCG_ERR_HIP, fn, "cannot make the context's device current");
    RolloutArgs R;
    fill_shared(c, R);
    R.x = a.x; R.y = a.y; R.vx = a.vx; R.vy = a.vy; R.option_id = a.option_id; R.opt_steps = a.opt_steps; R.ep_steps = a.ep_steps;
    R.qcache = a.qcache; R.action = a.action; R.reward = a.reward; R.done = a.done; R.W = a.W; R.clf = a.clf;
    if (a.stats) R.st = *a.stats;
    R.n_steps = a.n_steps;
    R.begin = (flags & SCG_ROLLOUT_BEGIN) ? 1u : 0u; R.one_episode = (flags & SCG_ROLLOUT_ONE_EPISODE) ? 1u : 0u;
    R.enabled = a.enabled_mask; R.t0 = a.t0;
    int epw;
    if (!rollout_epw(c, c->cfg.n_envs, epw)) return fail_in(c, SCG_ERR_INVALID, fn, "SCG_ROLLOUT_EPW must be 2, 4, 8, 16 or 32");
    R.epw = epw;
    if (a.pop_clf && !a.pop) return fail_in(c, SCG_ERR_INVALID, fn, "pop_clf without pop");      // SPEC §24.1: the last refusal
    if (a.pop_gate && !a.pop) return fail_in(c, SCG_ERR_INVALID, fn, "pop_gate without pop");     // SPEC §25.1: the last two refusals
    if (a.pop_gate && (intr || best))
        return fail_in(c, SCG_ERR_INVALID, fn, "pop_gate with SCG_SELECT_INTERRUPT or SCG_SELECT_BEST: the gate table is for the plain rules");
    const int wgs_per_pol = a.pop ? (a.pop->n_per + RO_WAVES * epw - 1) / (RO_WAVES * epw) : 0;
    const int grid = a.pop ? a.pop->n_policies * wgs_per_pol : (c->cfg.n_envs + RO_WAVES * epw - 1) / (RO_WAVES * epw);
    const hipStream_t s = reinterpret_cast<hipStream_t>(a.stream);
    c->order_valid = false;                               // the ids change under the step's prepared env order
    auto I = derived_args<RolloutIntArgs>(R);
    I.interrupts = a.interrupts;
    auto V = derived_args<RolloutVarArgs>(R);
    if (a.rec) V.rec = *a.rec;                            // (no rec: n = 0, nothing recorded)
    V.begin_at = at ? 1u : 0u;
    if (intr) V.interrupts = a.interrupts;
    if (best) V.overrides = a.overrides;
    if (audit) { V.au = *audit; V.gamma = c->cfg.gamma; }
    V.first_action = a.first_action;
    const bool aud = audit || a.first_action;             // the AUDIT kernels: they alone read first_action
    const bool var = aud || best || a.rec || at;          // what only the RolloutVar kernels take
    hipError_t rollout_kernel_launch = hipSuccess;
    if (a.pop) {
        auto P = derived_args<RolloutPopArgs>(V);
        P.n_pol = a.pop->n_policies; P.n_per = a.pop->n_per; P.wgs_per_pol = wgs_per_pol;
        P.pol_eps = a.pop->epsilon; P.pol_enabled = a.pop->enabled; P.pol_clf = a.pop_clf;
        if (a.pop_gate) {
            auto G = derived_args<RolloutPopGateArgs>(P);
            G.pol_gate = a.pop_gate;
            rollout_kernel_launch = launch_rollout<true>(G, grid, s);
        } else
        switch ((best ? 2 : 0) | (intr ? 1 : 0)) {
        case 0: rollout_kernel_launch = launch_rollout<true>(derived_args<RolloutPop<false, false>>(P), grid, s); break;
        case 1: rollout_kernel_launch = launch_rollout<true>(derived_args<RolloutPop<true, false>>(P), grid, s); break;
        case 2: rollout_kernel_launch = launch_rollout<true>(derived_args<RolloutPop<false, true>>(P), grid, s); break;
        case 3: rollout_kernel_launch = launch_rollout<true>(derived_args<RolloutPop<true, true>>(P), grid, s); break;
        }
    } else
    switch ((var ? 8 : 0) | (aud ? 4 : 0) | (best ? 2 : 0) | (intr ? 1 : 0)) {                      // INT    BEST   AUDIT
    case 0:
        hipLaunchKernelGGL((rollout_kernel<false, RolloutArgs>), dim3(grid), dim3(RO_THREADS), 0, s, R);
        rollout_kernel_launch = hipGetLastError();
        break;
    case 1: rollout_kernel_launch = launch_rollout<false, RolloutIntArgs>(I, grid, s); break;
    case 8: rollout_kernel_launch = launch_rollout<true>(derived_args<RolloutVar<false, false, false>>(V), grid, s); break;
    case 9: rollout_kernel_launch = launch_rollout<true>(derived_args<RolloutVar<true, false, false>>(V), grid, s); break;
    case 10: rollout_kernel_launch = launch_rollout<true>(derived_args<RolloutVar<false, true, false>>(V), grid, s); break;
    case 11: rollout_kernel_launch = launch_rollout<true>(derived_args<RolloutVar<true, true, false>>(V), grid, s); break;
    case 12: rollout_kernel_launch = launch_rollout<true>(derived_args<RolloutVar<false, false, true>>(V), grid, s); break;
    case 13: rollout_kernel_launch = launch_rollout<true>(derived_args<RolloutVar<true, false, true>>(V), grid, s); break;
    case 14: rollout_kernel_launch = launch_rollout<true>(derived_args<RolloutVar<false, true, true>>(V), grid, s); break;
    case 15: rollout_kernel_launch = launch_rollout<true>(derived_args<RolloutVar<true, true, true>>(V), grid, s); break;
    }
    SCG_HIP(c, rollout_kernel_launch);
    return SCG_OK;
}

int scg_rollout(scg_ctx *c, float *x, float *y, float *vx, float *vy, int32_t *option_id, int32_t *opt_steps,
                int32_t *ep_steps, float *qcache, uint8_t *action, float *reward, uint8_t *done,
                const float *W, const float *clf, uint32_t enabled_mask, uint64_t t0, int32_t n_steps,
                uint32_t flags, const scg_rollout_stats *stats, void *stream) {
    return rollout_launch("scg_rollout", c, {x, y, vx, vy, option_id, opt_steps, ep_steps, qcache, action, reward, done, W, clf,
                                             enabled_mask, t0, n_steps, flags, stats, stream});
}

int scg_rollout_record(scg_ctx *c, float *x, float *y, float *vx, float *vy, int32_t *option_id, int32_t *opt_steps,
                       int32_t *ep_steps, float *qcache, uint8_t *action, float *reward, uint8_t *done,
                       const float *W, const float *clf, uint32_t enabled_mask, uint64_t t0, int32_t n_steps,
                       uint32_t flags, const scg_rollout_stats *stats, const scg_record *rec, void *stream) {
    return rollout_launch("scg_rollout_record", c, {x, y, vx, vy, option_id, opt_steps, ep_steps, qcache, action, reward, done, W, clf,
                                                    enabled_mask, t0, n_steps, flags, stats, stream, true, rec});
}

int scg_rollout_interrupt(scg_ctx *c, float *x, float *y, float *vx, float *vy, int32_t *option_id, int32_t *opt_steps,
                          int32_t *ep_steps, float *qcache, uint8_t *action, float *reward, uint8_t *done,
                          const float *W, const float *clf, uint32_t enabled_mask, uint64_t t0, int32_t n_steps,
                          uint32_t flags, const scg_rollout_stats *stats, int32_t *interrupts, const scg_record *rec,
                          void *stream) {
    return rollout_launch("scg_rollout_interrupt", c, {x, y, vx, vy, option_id, opt_steps, ep_steps, qcache, action, reward, done, W, clf,
                                                       enabled_mask, t0, n_steps, flags, stats, stream, true, rec, interrupts, nullptr,
                                                       SCG_SELECT_INTERRUPT});
}

// rules = 0: scg_rollout_record's kernel; SCG_SELECT_INTERRUPT alone: scg_rollout_interrupt's
int scg_rollout_select(scg_ctx *c, float *x, float *y, float *vx, float *vy, int32_t *option_id, int32_t *opt_steps,
                       int32_t *ep_steps, float *qcache, uint8_t *action, float *reward, uint8_t *done,
                       const float *W, const float *clf, uint32_t enabled_mask, uint64_t t0, int32_t n_steps,
                       uint32_t flags, const scg_rollout_stats *stats, int32_t *interrupts, int32_t *overrides,
                       const scg_record *rec, uint32_t rules, void *stream) {
    return rollout_launch("scg_rollout_select", c, {x, y, vx, vy, option_id, opt_steps, ep_steps, qcache, action, reward, done, W, clf,
                                                    enabled_mask, t0, n_steps, flags, stats, stream, true, rec, interrupts, overrides,
                                                    rules});
}

// audit = NULL, or every member NULL: scg_rollout_select's launch, under this entry point's name in error texts
int scg_rollout_audit(scg_ctx *c, float *x, float *y, float *vx, float *vy, int32_t *option_id, int32_t *opt_steps,
                      int32_t *ep_steps, float *qcache, uint8_t *action, float *reward, uint8_t *done,
                      const float *W, const float *clf, uint32_t enabled_mask, uint64_t t0, int32_t n_steps,
                      uint32_t flags, const scg_rollout_stats *stats, int32_t *interrupts, int32_t *overrides,
                      const scg_record *rec, uint32_t rules, const scg_audit *audit, void *stream) {
    return rollout_launch("scg_rollout_audit", c, {x, y, vx, vy, option_id, opt_steps, ep_steps, qcache, action, reward, done, W, clf,
                                                   enabled_mask, t0, n_steps, flags, stats, stream, true, rec, interrupts, overrides,
                                                   rules, audit});
}

// first_action = NULL: scg_rollout_audit's launch, under this entry point's name in error texts
int scg_rollout_branch(scg_ctx *c, float *x, float *y, float *vx, float *vy, int32_t *option_id, int32_t *opt_steps,
                       int32_t *ep_steps, float *qcache, uint8_t *action, float *reward, uint8_t *done,
                       const float *W, const float *clf, uint32_t enabled_mask, uint64_t t0, int32_t n_steps,
                       uint32_t flags, const scg_rollout_stats *stats, int32_t *interrupts, int32_t *overrides,
                       const scg_record *rec, uint32_t rules, const scg_audit *audit, const uint8_t *first_action, void *stream) {
    return rollout_launch("scg_rollout_branch", c, {x, y, vx, vy, option_id, opt_steps, ep_steps, qcache, action, reward, done, W, clf,
                                                    enabled_mask, t0, n_steps, flags, stats, stream, true, rec, interrupts, overrides,
                                                    rules, audit, first_action});
}

// pop = NULL: scg_rollout_branch's launch, under this entry point's name in error texts
int scg_rollout_population(scg_ctx *c, float *x, float *y, float *vx, float *vy, int32_t *option_id, int32_t *opt_steps,
                           int32_t *ep_steps, float *qcache, uint8_t *action, float *reward, uint8_t *done,
                           const float *W, const float *clf, uint32_t enabled_mask, uint64_t t0, int32_t n_steps,
                           uint32_t flags, const scg_rollout_stats *stats, int32_t *interrupts, int32_t *overrides,
                           const scg_record *rec, uint32_t rules, const scg_audit *audit, const uint8_t *first_action, void *stream,
                           const scg_population *pop) {
    return scg_rollout_population_clf(c, x, y, vx, vy, option_id, opt_steps, ep_steps, qcache, action, reward, done, W, clf, enabled_mask,
                                      t0, n_steps, flags, stats, interrupts, overrides, rec, rules, audit, first_action, stream, pop,
                                      nullptr);
}

// pop_clf = NULL: scg_rollout_population's launch (and its name in error texts: they are one entry point with and without the table)
int scg_rollout_population_clf(scg_ctx *c, float *x, float *y, float *vx, float *vy, int32_t *option_id, int32_t *opt_steps,
                               int32_t *ep_steps, float *qcache, uint8_t *action, float *reward, uint8_t *done,
                               const float *W, const float *clf, uint32_t enabled_mask, uint64_t t0, int32_t n_steps,
                               uint32_t flags, const scg_rollout_stats *stats, int32_t *interrupts, int32_t *overrides,
                               const scg_record *rec, uint32_t rules, const scg_audit *audit, const uint8_t *first_action, void *stream,
                               const scg_population *pop, const float *pop_clf) {
    return scg_rollout_population_gate(c, x, y, vx, vy, option_id, opt_steps, ep_steps, qcache, action, reward, done, W, clf, enabled_mask,
                                       t0, n_steps, flags, stats, interrupts, overrides, rec, rules, audit, first_action, stream, pop,
                                       pop_clf, nullptr);
}

// pop_gate = NULL: scg_rollout_population_clf's launch, under the name that entry point gives in error texts
int scg_rollout_population_gate(scg_ctx *c, float *x, float *y, float *vx, float *vy, int32_t *option_id, int32_t *opt_steps,
                                int32_t *ep_steps, float *qcache, uint8_t *action, float *reward, uint8_t *done,
                                const float *W, const float *clf, uint32_t enabled_mask, uint64_t t0, int32_t n_steps,
                                uint32_t flags, const scg_rollout_stats *stats, int32_t *interrupts, int32_t *overrides,
                                const scg_record *rec, uint32_t rules, const scg_audit *audit, const uint8_t *first_action, void *stream,
                                const scg_population *pop, const float *pop_clf, const float *pop_gate) {
    return rollout_launch(pop_gate ? "scg_rollout_population_gate" : pop_clf ? "scg_rollout_population_clf" : "scg_rollout_population", c,
                          {x, y, vx, vy, option_id, opt_steps, ep_steps, qcache, action, reward, done, W, clf, enabled_mask, t0, n_steps, flags,
                           stats, stream, true, rec, interrupts, overrides, rules, audit, first_action, pop, pop_clf, pop_gate});
}

static int trials_launch(const char *fn, scg_ctx *c, int32_t n, const float *x, const float *y, const float *vx, const float *vy,
                         const int32_t *option, const float *W, const float *clf, uint32_t enabled_mask, uint64_t t0,
                         const scg_trial_out *out, const scg_record *rec, void *stream) {
    if (!c) return fail_in(nullptr, SCG_ERR_INVALID, fn, "null ctx");
    if (!c->have_map) return fail_in(c, SCG_ERR_STATE, fn, "scg_set_map has not been called");
    if (!x || !y || !vx || !vy || !option || !W || !clf || !out || !out->outcome)
        return fail_in(c, SCG_ERR_INVALID, fn, "null array argument (or out->outcome)");
    if (n < 1) return fail_in(c, SCG_ERR_INVALID, fn, "n must be >= 1");
    if (std::min(c->cfg.max_option_steps, c->cfg.max_episode_steps) > SCG_TRIAL_MAX_STEPS)
        return fail_in(c, SCG_ERR_INVALID, fn, "min(max_option_steps, max_episode_steps) exceeds SCG_TRIAL_MAX_STEPS");
    if (rec) {
        const int rc = check_record(c, fn, rec, n, 1);
        if (rc != SCG_OK) return rc;
    }
    SCG_CHECK_ASYNC(c);
    DeviceGuard dev_guard_(c->cfg.device);
    if (!dev_guard_.ok) return fail_in(c, SCG_ERR_HIP, fn, "cannot make the context's device current");
    TrialArgs T;
    fill_shared(c, T);
    T.n = n;
    T.x = x; T.y = y; T.vx = vx; T.vy = vy; T.option = option; T.out = *out; T.W = W; T.clf = clf;
    T.enabled = enabled_mask; T.t0 = t0;
    T.gamma = c->cfg.gamma; T.r_succ = c->cfg.r_option_success;
    int epw;
    if (!rollout_epw(c, n, epw)) return fail_in(c, SCG_ERR_INVALID, fn, "SCG_ROLLOUT_EPW must be 2, 4, 8, 16 or 32");
    T.epw = epw;
    const int grid = (int)(((long long)n + RO_WAVES * epw - 1) / (RO_WAVES * epw));
    if (rec) {
        auto TR = derived_args<TrialRecArgs>(T);
        TR.rec = *rec;
        SCG_HIP(c, launch_trial_record(TR, grid, reinterpret_cast<hipStream_t>(stream)));
    } else {
        hipLaunchKernelGGL((trial_kernel<false, TrialArgs>), dim3(grid), dim3(RO_THREADS), 0, reinterpret_cast<hipStream_t>(stream), T);
        SCG_HIP(c, hipGetLastError());
    }
    return SCG_OK;
}

int scg_option_trials(scg_ctx *c, int32_t n, const float *x, const float *y, const float *vx, const float *vy,
                      const int32_t *option, const float *W, const float *clf, uint32_t enabled_mask, uint64_t t0,
                      const scg_trial_out *out, void *stream) {
    return trials_launch("scg_option_trials", c, n, x, y, vx, vy, option, W, clf, enabled_mask, t0, out, nullptr, stream);
}

int scg_option_trials_record(scg_ctx *c, int32_t n, const float *x, const float *y, const float *vx, const float *vy,
                             const int32_t *option, const float *W, const float *clf, uint32_t enabled_mask, uint64_t t0,
                             const scg_trial_out *out, const scg_record *rec, void *stream) {
    return trials_launch("scg_option_trials_record", c, n, x, y, vx, vy, option, W, clf, enabled_mask, t0, out, rec, stream);
}

int scg_invalidate_order(scg_ctx *c) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_invalidate_order: null ctx");
    c->order_valid = false;
    return SCG_OK;
}

#ifdef SCG_STAMPS_LITE
extern "C" int scg_diag_stamps(scg_ctx *c, unsigned long long *host_out /*[nblk][STAMP_SLOTS]*/, int32_t reset) {
    if (!c || !c->d_stamps) return SCG_ERR_STATE;
    if (host_out && hipMemcpy(host_out, c->d_stamps, (size_t)c->nblk * STAMP_SLOTS * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return SCG_ERR_HIP;
    if (reset) (void)hipMemset(c->d_stamps, 0, (size_t)c->nblk * STAMP_SLOTS * sizeof(unsigned long long));
    return SCG_OK;
}
#endif

#ifdef SCG_REDUCE_STAMPS
// the last reduce launch's workgroup stamps, [RED_NCOL * (n_vf + row slots)][RED_STAMP_SLOTS] in grid order (y major); returns the workgroup count
extern "C" int scg_diag_reduce_stamps(scg_ctx *c, unsigned long long *host_out, int32_t reset) {
    if (!c || !c->d_stamps) return -1;
    if (host_out && hipMemcpy(host_out, c->d_stamps, reduce_stamp_bytes(c), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (reset) (void)hipMemset(c->d_stamps, 0, reduce_stamp_bytes(c));
    return (int)(reduce_stamp_bytes(c) / (RED_STAMP_SLOTS * sizeof(unsigned long long)));
}
#endif

int scg_set_option_parents(scg_ctx *c, const int32_t *parents) {
    if (!c || !parents) return fail(c, SCG_ERR_INVALID, "scg_set_option_parents: null argument");
    uint32_t packed = 0;
    for (int k = 1; k <= c->cfg.n_options; ++k) {
        if (parents[k] < 0 || parents[k] > c->cfg.n_options || parents[k] == k)
            return fail(c, SCG_ERR_INVALID, "scg_set_option_parents: parent must be 0 (goal) or another option");
        packed |= (uint32_t)parents[k] << (3 * k);
    }
    for (int k = 1; k <= c->cfg.n_options; ++k) {          // no cycles: following parents must reach the goal
        int p = k, hops = 0;
        while (p != 0 && hops <= SCG_MAX_OPTIONS) { p = parents[p]; ++hops; }
        if (p != 0) return fail(c, SCG_ERR_INVALID, "scg_set_option_parents: the option graph has a cycle");
    }
    c->parents = packed;
    return SCG_OK;
}

int scg_set_gestation(scg_ctx *c, uint32_t gest_mask, int32_t *succ_counts) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_set_gestation: null ctx");
    if (gest_mask & ~(((1u << c->n_vf) - 1u) & ~1u)) return fail(c, SCG_ERR_INVALID, "scg_set_gestation: mask names no option of this context");
    c->gest = gest_mask; c->gest_succ = succ_counts;
    return SCG_OK;
}

int scg_collect_examples(scg_ctx *c, uint32_t event_bits, uint8_t *prev_in, int32_t l_pos, int32_t l_neg, float *ex_xy,
                         uint8_t *ex_label, int32_t *count, int32_t cap, void *stream) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_collect_examples: null ctx");
    if (!c->ring_x || !c->events) return fail(c, SCG_ERR_STATE, "scg_collect_examples: trace buffers are not attached");
    if (!event_bits || bad_window(l_pos, l_neg) || !ex_xy || !ex_label || !count || cap < 0)
        return fail(c, SCG_ERR_INVALID, "scg_collect_examples: bad argument");
    SCG_CHECK_ASYNC(c);
    SCG_ON_DEVICE(c, "scg_collect_examples");
    const int nrows = (c->cfg.n_envs + COL_ROW - 1) / COL_ROW;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool have_rows = c->arm_rows_ready && c->arm_bits == event_bits && c->arm_prev == prev_in && c->arm_count == count &&
                           c->arm_L == l_pos + l_neg;
    c->arm_rows_ready = false;                               // prev_in changes below: the totals are used up
    if (!have_rows)
    hipLaunchKernelGGL(collect_count_kernel, dim3(nrows), dim3(COL_ROW), 0, s, c->cfg.n_envs, c->events, prev_in, event_bits,
                       c->ev_len, c->ring_len, l_pos + l_neg, c->d_collect_rows, nrows, count);
    hipLaunchKernelGGL(collect_scatter_kernel, dim3(nrows), dim3(COL_ROW), 0, s, c->cfg.n_envs, c->events, prev_in, event_bits,
                       c->ring_x, c->ring_y, c->ring_len, c->ev_len, l_pos, l_neg, ex_xy, ex_label, count, cap,
                       c->d_collect_rows, nrows);
    SCG_HIP(c, hipGetLastError());
    return SCG_OK;
}

int scg_collect_frontier(scg_ctx *c, uint32_t target_mask, uint32_t cover_mask, const float *clf, int32_t l_pos, int32_t l_neg,
                         float *ex_xy, uint8_t *ex_label, int32_t *count, int32_t cap, void *stream) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_collect_frontier: null ctx");
    if (!c->ring_x || !c->events) return fail(c, SCG_ERR_STATE, "scg_collect_frontier: trace buffers are not attached");
    const uint32_t nodes = (1u << c->n_vf) - 1u, opts = nodes & ~1u;
    if (target_mask & ~nodes) return fail(c, SCG_ERR_INVALID, "scg_collect_frontier: target_mask names no node of this context");
    if (cover_mask & ~opts) return fail(c, SCG_ERR_INVALID, "scg_collect_frontier: cover_mask must name options 1..n_options only");
    if (target_mask & opts & ~cover_mask)
        return fail(c, SCG_ERR_INVALID, "scg_collect_frontier: a target option must be part of the cover");
    if (cap < 1 || bad_window(l_pos, l_neg) || !clf || !ex_xy || !ex_label || !count)
        return fail(c, SCG_ERR_INVALID, "scg_collect_frontier: bad argument");
    SCG_CHECK_ASYNC(c);
    SCG_ON_DEVICE(c, "scg_collect_frontier");
    if (!target_mask) return SCG_OK;                         // no node: nothing to append
    const int nrows = (c->cfg.n_envs + COL_ROW - 1) / COL_ROW;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(frontier_count_kernel, dim3(nrows), dim3(COL_ROW), 0, s, c->cfg.n_envs, c->events, c->ev_len, c->ring_x,
                       c->ring_y, c->ring_len, clf, c->n_vf, target_mask, cover_mask, l_pos + l_neg, c->d_frontier_rows, nrows,
                       count);
    hipLaunchKernelGGL(frontier_scatter_kernel, dim3(nrows), dim3(COL_ROW), 0, s, c->cfg.n_envs, c->events, c->ev_len, c->ring_x,
                       c->ring_y, c->ring_len, clf, c->n_vf, target_mask, cover_mask, l_pos, l_neg, ex_xy, ex_label, count, cap,
                       c->d_frontier_rows, nrows);
    SCG_HIP(c, hipGetLastError());
    return SCG_OK;
}

int scg_arm_collect(scg_ctx *c, uint32_t event_bits, const uint8_t *prev_in, int32_t l_pos, int32_t l_neg, const int32_t *count) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_arm_collect: null ctx");
    c->arm_rows_ready = false;
    if (event_bits == 0) { c->arm_bits = 0; return SCG_OK; }
    if (bad_window(l_pos, l_neg) || !count)
        return fail(c, SCG_ERR_INVALID, "scg_arm_collect: bad argument");
    if (!c->ring_x || !c->events) return fail(c, SCG_ERR_STATE, "scg_arm_collect: trace buffers are not attached");
    c->arm_bits = event_bits; c->arm_prev = prev_in; c->arm_count = count; c->arm_L = l_pos + l_neg;
    return SCG_OK;
}

int scg_set_trace_buffers(scg_ctx *c, float *ring_x, float *ring_y, int32_t ring_len, uint8_t *events,
                          int32_t *ev_len) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_set_trace_buffers: null ctx");
    c->arm_bits = 0; c->arm_rows_ready = false;             // an announced trigger refers to the old buffers
    if ((ring_x == nullptr) != (ring_y == nullptr)) return fail(c, SCG_ERR_INVALID, "scg_set_trace_buffers: ring_x and ring_y go together");
    if (ring_x && !pow2(ring_len)) return fail(c, SCG_ERR_INVALID, "scg_set_trace_buffers: ring_len must be a power of two");
    if ((events == nullptr) != (ev_len == nullptr)) return fail(c, SCG_ERR_INVALID, "scg_set_trace_buffers: events and ev_len go together");
    c->ring_x = ring_x; c->ring_y = ring_y; c->ring_len = ring_x ? ring_len : 0; c->events = events; c->ev_len = ev_len;
    return SCG_OK;
}

int scg_harvest(scg_ctx *c, int32_t n_sel, const int32_t *sel_env, const float *ring_x, const float *ring_y,
                int32_t ring_len, const int32_t *ev_len, int32_t l_pos, int32_t l_neg, float *out_xy,
                uint8_t *out_label, void *stream) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_harvest: null ctx");
    if (n_sel < 0 || bad_window(l_pos, l_neg) || !pow2(ring_len) || !sel_env || !ring_x || !ring_y || !ev_len || !out_xy || !out_label)
        return fail(c, SCG_ERR_INVALID, "scg_harvest: bad argument");
    SCG_CHECK_ASYNC(c);
    SCG_ON_DEVICE(c, "scg_harvest");
    if (n_sel == 0) return SCG_OK;
    const long long total = (long long)n_sel * (l_pos + l_neg);
    hipLaunchKernelGGL(harvest_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), n_sel, sel_env, ring_x, ring_y, ring_len, c->cfg.n_envs,
                       ev_len, l_pos, l_neg, out_xy, out_label);
    SCG_HIP(c, hipGetLastError());
    return SCG_OK;
}

int scg_profile_reset(scg_ctx *c, int32_t enable) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_profile_reset: null ctx");
    c->prof_on = enable > 0;
    c->prof_every = enable > 0 ? enable : 1;
    c->prof_seen = 0;
    c->prof_used = 0;
    if (enable > 0) {                       // a pool of events up front: creating them lazily cost the first sampled launches of a
        SCG_ON_DEVICE(c, "scg_profile_reset");      // timed region tens of microseconds of host time in front of an idle queue
        if (!c->prof_ev) c->prof_ev = new std::vector<hipEvent_t>();
        while (c->prof_ev->size() < 64) {
            hipEvent_t e;
            SCG_HIP(c, hipEventCreate(&e));
            c->prof_ev->push_back(e);
        }
    }
    return SCG_OK;
}

int scg_profile_read(scg_ctx *c, double *kernel_ms_sum, int64_t *launches) {
    if (!c || !kernel_ms_sum || !launches) return fail(c, SCG_ERR_INVALID, "scg_profile_read: null argument");
    double sum = 0.0;
    for (size_t i = 0; i + 1 < c->prof_used; i += 2) {
        SCG_HIP(c, hipEventSynchronize((*c->prof_ev)[i + 1]));
        float ms = 0.0f;
        SCG_HIP(c, hipEventElapsedTime(&ms, (*c->prof_ev)[i], (*c->prof_ev)[i + 1]));
        sum += ms;
    }
    *kernel_ms_sum = sum;
    *launches = (int64_t)(c->prof_used / 2);
    return SCG_OK;
}

int scg_grad_buffers(scg_ctx *c, float **G, int32_t **n_k) {
    if (!c || !G || !n_k) return fail(c, SCG_ERR_INVALID, "scg_grad_buffers: null argument");
    *G = c->G_out; *n_k = c->nk_out;
    return SCG_OK;
}

int scg_set_grad_buffers(scg_ctx *c, float *G, int32_t *n_k) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_set_grad_buffers: null ctx");
    if ((G == nullptr) != (n_k == nullptr))
        return fail(c, SCG_ERR_INVALID, "scg_set_grad_buffers: pass both buffers or neither");
    c->G_out = G ? G : c->d_G;
    c->nk_out = n_k ? n_k : c->d_nk;
    c->nkf_out = nullptr;
    return SCG_OK;
}

int scg_set_grad_buffer_packed(scg_ctx *c, float *G_packed) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_set_grad_buffer_packed: null ctx");
    c->G_out = G_packed ? G_packed : c->d_G;
    c->nk_out = c->d_nk;
    c->nkf_out = G_packed ? G_packed + (size_t)c->n_vf * NACT * NF : nullptr;
    return SCG_OK;
}

int scg_apply_update_packed(scg_ctx *c, float *W, const float *G_packed, void *stream) {
    if (!c || !W || !G_packed) return fail(c, SCG_ERR_INVALID, "scg_apply_update_packed: null argument");
    if (!c->have_map) return fail(c, SCG_ERR_STATE, "scg_apply_update_packed: scg_set_map has not been called (scale table)");
    SCG_CHECK_ASYNC(c);
    SCG_ON_DEVICE(c, "scg_apply_update_packed");
    dim3 grid((NACT * NF + 255) / 256, c->n_vf);
    hipLaunchKernelGGL(apply_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), W, G_packed,
                       (const int32_t *)nullptr, G_packed + (size_t)c->n_vf * NACT * NF, c->d_scale, c->cfg.alpha, c->cfg.update_count_floor);
    SCG_HIP(c, hipGetLastError());
    return SCG_OK;
}

int scg_apply_update_slots(scg_ctx *c, float *W, const float *slots, int32_t n_slots, int64_t slot_stride, void *stream) {
    if (!c || !W || !slots) return fail(c, SCG_ERR_INVALID, "scg_apply_update_slots: null argument");
    if (n_slots < 1 || n_slots > 4096 || slot_stride < (int64_t)c->n_vf * NACT * NF + c->n_vf)
        return fail(c, SCG_ERR_INVALID, "scg_apply_update_slots: n_slots must be in [1, 4096] and slot_stride >= n_vf * 6480 + n_vf floats");
    if (!c->have_map) return fail(c, SCG_ERR_STATE, "scg_apply_update_slots: scg_set_map has not been called (scale table)");
    SCG_CHECK_ASYNC(c);
    SCG_ON_DEVICE(c, "scg_apply_update_slots");
    dim3 grid((NACT * NF + 255) / 256, c->n_vf);
    hipLaunchKernelGGL(apply_slots_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), W, slots, (int)n_slots,
                       (long)slot_stride, c->n_vf, c->d_scale, c->cfg.alpha, c->cfg.update_count_floor);
    SCG_HIP(c, hipGetLastError());
    return SCG_OK;
}

int scg_peer_export(scg_ctx *c, void *handle_out) {
    if (!c || !handle_out) return fail(c, SCG_ERR_INVALID, "scg_peer_export: null argument");
    if (!c->peer_region) {
        SCG_ON_DEVICE(c, "scg_peer_export");
        const size_t op = ((size_t)c->n_vf * NACT * NF + c->n_vf) * sizeof(float);
        c->peer_op_stride = (op + 255) & ~(size_t)255;
        c->peer_bytes = PEER_HDR + 2 * c->peer_op_stride;
        char *r = nullptr;
        SCG_HIP(c, hipMalloc(reinterpret_cast<void **>(&r), c->peer_bytes));        // ONE allocation: an IPC handle names it whole
        hipIpcMemHandle_t h;
        if (hipMemset(r, 0, c->peer_bytes) != hipSuccess || hipMalloc(&c->d_peer_go, sizeof(int32_t)) != hipSuccess ||
            hipIpcGetMemHandle(&h, r) != hipSuccess) {
            (void)hipFree(r); (void)hipFree(c->d_peer_go); c->d_peer_go = nullptr;
            return fail(c, SCG_ERR_HIP, "scg_peer_export: cannot allocate / export the peer region");
        }
        c->peer_region = r; c->peer_handle = h;
        std::lock_guard<std::mutex> lk(g_peer_mu);
        g_peer_regions.emplace_back(h, r);
    }
    memcpy(handle_out, &c->peer_handle, sizeof(hipIpcMemHandle_t));
    return SCG_OK;
}

int scg_peer_open(scg_ctx *c, int32_t n_ranks, int32_t rank, const void *handles) {
    if (!c || !handles) return fail(c, SCG_ERR_INVALID, "scg_peer_open: null argument");
    if (n_ranks < 1 || n_ranks > PEER_MAX || rank < 0 || rank >= n_ranks)
        return fail(c, SCG_ERR_INVALID, "scg_peer_open: n_ranks must be in [1, 8] and rank in [0, n_ranks)");
    if (!c->peer_region) return fail(c, SCG_ERR_STATE, "scg_peer_open: scg_peer_export has not been called");
    if (c->peer_n) return fail(c, SCG_ERR_STATE, "scg_peer_open: the peers are already open");
    SCG_ON_DEVICE(c, "scg_peer_open");
    const hipIpcMemHandle_t *hs = reinterpret_cast<const hipIpcMemHandle_t *>(handles);
    char *base[PEER_MAX] = {};
    bool mapped[PEER_MAX] = {};
    int st = SCG_OK;
    for (int r = 0; r < n_ranks && st == SCG_OK; ++r) {
        if (r == rank) {
            if (memcmp(&hs[r], &c->peer_handle, sizeof(hipIpcMemHandle_t)) != 0)
                st = fail(c, SCG_ERR_INVALID, "scg_peer_open: handles[rank] is not this context's region");
            base[r] = c->peer_region;
            continue;
        }
        {
            std::lock_guard<std::mutex> lk(g_peer_mu);
            for (auto &e : g_peer_regions)
                if (memcmp(&e.first, &hs[r], sizeof(hipIpcMemHandle_t)) == 0) base[r] = e.second;
        }
        if (base[r]) continue;                                   // a peer context of this process
        void *p = nullptr;
        if (hipIpcOpenMemHandle(&p, hs[r], hipIpcMemLazyEnablePeerAccess) != hipSuccess) {
            snprintf(c->err, sizeof(c->err), "scg_peer_open: hipIpcOpenMemHandle of rank %d failed: %s", r,
                     hipGetErrorString(hipGetLastError()));
            st = SCG_ERR_HIP;
            break;
        }
        base[r] = static_cast<char *>(p); mapped[r] = true;
    }
    if (st != SCG_OK) {
        for (int r = 0; r < n_ranks; ++r)
            if (mapped[r]) (void)hipIpcCloseMemHandle(base[r]);
        return st;
    }
    for (int r = 0; r < PEER_MAX; ++r) { c->peer_base[r] = base[r]; c->peer_mapped[r] = mapped[r]; }
    c->peer_n = n_ranks; c->peer_rank = rank;
    return SCG_OK;
}

int scg_peer_exchange_apply(scg_ctx *c, float *W, void *stream) {
    if (!c || !W) return fail(c, SCG_ERR_INVALID, "scg_peer_exchange_apply: null argument");
    if (!c->peer_n) return fail(c, SCG_ERR_STATE, "scg_peer_exchange_apply: scg_peer_open has not been called");
    if (!c->have_map) return fail(c, SCG_ERR_STATE, "scg_peer_exchange_apply: scg_set_map has not been called (scale table)");
    // A pending failure does NOT stop the exchange: the peers wait for this rank's epoch, and a voided step must reach them
    // as a void flag (no rank applies), not as a timeout. The failure is reported after the launches.
    const bool pending = async_pending(c) != 0;
    char why[256];
    memcpy(why, c->err, sizeof(why));
    SCG_ON_DEVICE(c, "scg_peer_exchange_apply");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PeerView P;
    memset(&P, 0, sizeof(P));
    for (int r = 0; r < c->peer_n; ++r) {
        P.epoch[r] = reinterpret_cast<const uint32_t *>(c->peer_base[r]);
        P.voidw[r] = reinterpret_cast<const uint32_t *>(c->peer_base[r] + 128);
        for (int p = 0; p < 2; ++p) P.buf[r][p] = reinterpret_cast<const float *>(c->peer_base[r] + PEER_HDR + p * c->peer_op_stride);
    }
    const int parity = (int)(c->peer_e & 1u);
    const uint32_t need = c->peer_e + 1u;
    hipLaunchKernelGGL(peer_publish_kernel, dim3(1), dim3(64), 0, s, reinterpret_cast<uint32_t *>(c->peer_region),
                       reinterpret_cast<uint32_t *>(c->peer_region + 128), parity, (const int32_t *)c->d_fail, need);
    SCG_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(peer_wait_kernel, dim3(1), dim3(64), 0, s, P, c->peer_n, parity, need,
                       (unsigned long long)(c->peer_timeout_s * 1e8), c->d_peer_go, c->d_async);
    SCG_HIP(c, hipGetLastError());
    dim3 grid((NACT * NF + 255) / 256, c->n_vf);
    hipLaunchKernelGGL(apply_peers_kernel, grid, dim3(256), 0, s, W, P, c->peer_n, parity, need, (const int32_t *)c->d_peer_go,
                       c->n_vf, c->d_scale, c->cfg.alpha, c->cfg.update_count_floor);
    SCG_HIP(c, hipGetLastError());
    c->peer_e += 1u;
    if (pending) { memcpy(c->err, why, sizeof(why)); return SCG_ERR_ASYNC; }
    return SCG_OK;
}

int scg_apply_update(scg_ctx *c, float *W, const float *G, const int32_t *n_k, void *stream) {
    if (!c || !W || !G || !n_k) return fail(c, SCG_ERR_INVALID, "scg_apply_update: null argument");
    if (!c->have_map) return fail(c, SCG_ERR_STATE, "scg_apply_update: scg_set_map has not been called (scale table)");
    SCG_CHECK_ASYNC(c);
    SCG_ON_DEVICE(c, "scg_apply_update");
    dim3 grid((NACT * NF + 255) / 256, c->n_vf);
    hipLaunchKernelGGL(apply_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), W, G, n_k,
                       (const float *)nullptr, c->d_scale, c->cfg.alpha, c->cfg.update_count_floor);
    SCG_HIP(c, hipGetLastError());
    return SCG_OK;
}

int scg_pinball_step(scg_ctx *c, int32_t n, float *x, float *y, float *vx, float *vy, const uint8_t *action,
                     float *reward, uint8_t *goal, void *stream) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_pinball_step: null ctx");
    if (!c->have_map) return fail(c, SCG_ERR_STATE, "scg_pinball_step: scg_set_map has not been called");
    if (n < 0 || !x || !y || !vx || !vy || !action || !reward || !goal)
        return fail(c, SCG_ERR_INVALID, "scg_pinball_step: bad argument");
    SCG_CHECK_ASYNC(c);
    SCG_ON_DEVICE(c, "scg_pinball_step");
    if (n == 0) return SCG_OK;
    hipLaunchKernelGGL(pinball_kernel, dim3((n + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       n, x, y, vx, vy, action, reward, goal, c->d_edges, c->d_cellmask, c->ms);
    SCG_HIP(c, hipGetLastError());
    return SCG_OK;
}

int scg_fourier_features(scg_ctx *c, int32_t n, const float *x, const float *y, const float *vx,
                         const float *vy, float *phi, void *stream) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_fourier_features: null ctx");
    if (n < 0 || !x || !y || !vx || !vy || !phi) return fail(c, SCG_ERR_INVALID, "scg_fourier_features: bad argument");
    SCG_CHECK_ASYNC(c);
    SCG_ON_DEVICE(c, "scg_fourier_features");
    if (n == 0) return SCG_OK;
    const int grid = n < 8192 ? n : 8192;
    hipLaunchKernelGGL(features_kernel, dim3(grid), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), n, x, y,
                       vx, vy, phi);
    SCG_HIP(c, hipGetLastError());
    return SCG_OK;
}

// What scg_feature_gram, scg_feature_gram_targets and scg_feature_cross_gram share behind their null checks: the other argument
// checks, an empty segment's +0 fill, the non-empty segments listed into G — as listed, or longest first (ties as listed: blockIdx.y is dispatched slowest, so the
// longest chains start first) — and the launch. G's pointers are the caller's; F is the feature count of the launch's order (§18);
// n_tgt the right-hand sides a segment has in G.b (1 but for scg_feature_gram_targets, whose range check is the last one, and for
// scg_feature_gram_weighted — `weighted` —, whose range starts at 0 and whose Y and B, given or not as n_tgt says, are checked behind it).
static int gram_call(scg_ctx *c, const char *fn, bool null_array, bool yv_without_b, int64_t n, int32_t n_seg, const int64_t *offsets,
                     int F, GramArgs &G, bool longest_first, hipError_t (*launch)(const GramArgs &, int, hipStream_t), void *stream,
                     int32_t n_tgt = 1, bool weighted = false) {
    if (!c) return fail_in(nullptr, SCG_ERR_INVALID, fn, "null ctx");
    if (null_array) return fail_in(c, SCG_ERR_INVALID, fn, "null array argument");
    if (n < 0) return fail_in(c, SCG_ERR_INVALID, fn, "n must be >= 0");
    if (n_seg < 1 || n_seg > SCG_GRAM_MAX_SEGMENTS) return fail_in(c, SCG_ERR_INVALID, fn, "n_seg out of range [1, SCG_GRAM_MAX_SEGMENTS]");
    if (yv_without_b) return fail_in(c, SCG_ERR_INVALID, fn, "yv and b go together");
    if (offsets[0] < 0 || offsets[n_seg] > n) return fail_in(c, SCG_ERR_INVALID, fn, "offsets leave [0, n]");
    for (int g = 0; g < n_seg; ++g)
        if (offsets[g + 1] < offsets[g]) return fail_in(c, SCG_ERR_INVALID, fn, "offsets decrease");
    if (weighted) {
        if (n_tgt < 0 || n_tgt > SCG_GRAM_MAX_TARGETS) return fail_in(c, SCG_ERR_INVALID, fn, "n_tgt out of range [0, SCG_GRAM_MAX_TARGETS]");
        if (n_tgt == 0 && (G.yv || G.b)) return fail_in(c, SCG_ERR_INVALID, fn, "n_tgt = 0 goes with a null Y and a null B");
        if (n_tgt >= 1 && (!G.yv || !G.b)) return fail_in(c, SCG_ERR_INVALID, fn, "n_tgt >= 1 needs Y and B");
    } else if (n_tgt < 1 || n_tgt > SCG_GRAM_MAX_TARGETS) return fail_in(c, SCG_ERR_INVALID, fn, "n_tgt out of range [1, SCG_GRAM_MAX_TARGETS]");
    SCG_CHECK_ASYNC(c);
    DeviceGuard dev_guard(c->cfg.device);
    if (!dev_guard.ok) return fail_in(c, SCG_ERR_HIP, fn, "cannot make the context's device current");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int n_active = 0;
    for (int g = 0; g < n_seg; ++g) {
        const int64_t cnt = offsets[g + 1] - offsets[g];
        if (cnt > 0) {
            int at = n_active++;
            for (; longest_first && at > 0 && G.count[at - 1] < cnt; --at) { G.seg[at] = G.seg[at - 1]; G.start[at] = G.start[at - 1]; G.count[at] = G.count[at - 1]; }
            G.seg[at] = g; G.start[at] = offsets[g]; G.count[at] = cnt;
        } else {                                          // an empty segment: all +0 (the kernel writes every entry of the others)
            SCG_HIP(c, hipMemsetAsync(G.out + (size_t)g * F * F, 0, (size_t)F * F * sizeof(float), s));
            if (G.b) SCG_HIP(c, hipMemsetAsync(G.b + (size_t)g * n_tgt * F, 0, (size_t)n_tgt * F * sizeof(float), s));
        }
    }
    for (int g = n_active; g < GRAM_MAX_SEG; ++g) { G.seg[g] = 0; G.start[g] = 0; G.count[g] = 0; }
    if (n_active) SCG_HIP(c, launch(G, n_active, s));
    return SCG_OK;
}

int scg_feature_gram(scg_ctx *c, int64_t n, const float *x, const float *y, const float *vx, const float *vy, const float *yv,
                     int32_t n_seg, const int64_t *offsets, float *A, float *b, void *stream) {
    GramArgs G = {{{x, y, vx, vy}, {x, y, vx, vy}}, yv, A, b};
    return gram_call(c, "scg_feature_gram", !x || !y || !vx || !vy || !A || !offsets, (yv == nullptr) != (b == nullptr), n, n_seg, offsets,
                     NF, G, false, launch_feature_gram, stream);
}

// SPEC §20.1: Y's n_tgt targets fill the columns of the B operand that carries scg_feature_gram's yv
int scg_feature_gram_targets(scg_ctx *c, int64_t n, const float *x, const float *y, const float *vx, const float *vy, const float *Y,
                             int32_t n_tgt, int32_t n_seg, const int64_t *offsets, float *A, float *B, void *stream) {
    GramArgs G = {{{x, y, vx, vy}, {x, y, vx, vy}}, Y, A, B};
    G.y_stride = n; G.n_tgt = n_tgt;
    return gram_call(c, "scg_feature_gram_targets", !x || !y || !vx || !vy || !Y || !A || !B || !offsets, false, n, n_seg, offsets,
                     NF, G, false, launch_feature_gram_targets, stream, n_tgt);
}

// SPEC §22.1: every operand of scg_feature_gram_targets' kernel times the sample's root weight
int scg_feature_gram_weighted(scg_ctx *c, int64_t n, const float *x, const float *y, const float *vx, const float *vy, const float *rw,
                              const float *Y, int32_t n_tgt, int32_t n_seg, const int64_t *offsets, float *A, float *B, void *stream) {
    GramArgs G = {{{x, y, vx, vy}, {x, y, vx, vy}}, Y, A, B};
    G.y_stride = n; G.n_tgt = n_tgt; G.rw = rw;
    return gram_call(c, "scg_feature_gram_weighted", !x || !y || !vx || !vy || !rw || !A || !offsets, false, n, n_seg, offsets,
                     NF, G, false, launch_feature_gram_weighted, stream, n_tgt, true);
}

int scg_feature_cross_gram(scg_ctx *c, int64_t n, const float *x, const float *y, const float *vx, const float *vy,
                           const float *x2, const float *y2, const float *vx2, const float *vy2,
                           int32_t n_seg, const int64_t *offsets, float *Cm, void *stream) {
    GramArgs G = {{{x, y, vx, vy}, {x2, y2, vx2, vy2}}, nullptr, Cm, nullptr};
    return gram_call(c, "scg_feature_cross_gram", !x || !y || !vx || !vy || !x2 || !y2 || !vx2 || !vy2 || !Cm || !offsets, false, n, n_seg,
                     offsets, NF, G, true, launch_feature_cross_gram, stream);
}

// ---- SPEC §18: the basis-order probe. A null ctx is refused first, then an order outside {3, 5, 7}; order 5 goes to the kernels above.
static int basis_order_features(int32_t order) { return order == 3 ? 256 : (order == 5 ? NF : (order == 7 ? 4096 : 0)); }

int scg_basis_features(scg_ctx *c, int32_t order, int64_t n, const float *x, const float *y, const float *vx, const float *vy,
                       float *phi, void *stream) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_basis_features: null ctx");
    if (!basis_order_features(order)) return fail(c, SCG_ERR_INVALID, "scg_basis_features: order must be 3, 5 or 7");
    if (n < 0 || !x || !y || !vx || !vy || !phi) return fail(c, SCG_ERR_INVALID, "scg_basis_features: bad argument");
    SCG_CHECK_ASYNC(c);
    SCG_ON_DEVICE(c, "scg_basis_features");
    if (n == 0) return SCG_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (order == 5) {
        if (n > INT32_MAX) return fail(c, SCG_ERR_INVALID, "scg_basis_features: n must fit 32 bits at order 5");
        hipLaunchKernelGGL(features_kernel, dim3(n < 8192 ? (int)n : 8192), dim3(64), 0, s, (int)n, x, y, vx, vy, phi);
        SCG_HIP(c, hipGetLastError());
    } else {
        const float *st[4] = {x, y, vx, vy};
        SCG_HIP(c, launch_basis_features(order, n, st, phi, s));
    }
    return SCG_OK;
}

int scg_basis_gram(scg_ctx *c, int32_t order, int64_t n, const float *x, const float *y, const float *vx, const float *vy,
                   const float *yv, int32_t n_seg, const int64_t *offsets, float *A, float *b, void *stream) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_basis_gram: null ctx");
    const int F = basis_order_features(order);
    if (!F) return fail(c, SCG_ERR_INVALID, "scg_basis_gram: order must be 3, 5 or 7");
    GramArgs G = {{{x, y, vx, vy}, {x, y, vx, vy}}, yv, A, b};
    return gram_call(c, "scg_basis_gram", !x || !y || !vx || !vy || !A || !offsets, (yv == nullptr) != (b == nullptr), n, n_seg, offsets,
                     F, G, false, order == 3 ? launch_basis_gram_3 : (order == 5 ? launch_feature_gram : launch_basis_gram_7), stream);
}

// ---- SPEC §23: the instruments of the Fourier initiation classifier's IRLS fit
int scg_logistic_terms(scg_ctx *c, int64_t n, const float *z, const uint8_t *label, float *p, float *rw, float *e, void *stream) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_logistic_terms: null ctx");
    if (n < 0) return fail(c, SCG_ERR_INVALID, "scg_logistic_terms: n must be >= 0");
    if (!z || !label || !p || !rw || !e) return fail(c, SCG_ERR_INVALID, "scg_logistic_terms: null array argument");
    SCG_CHECK_ASYNC(c);
    SCG_ON_DEVICE(c, "scg_logistic_terms");
    if (n == 0) return SCG_OK;
    SCG_HIP(c, launch_logistic_terms(n, z, label, p, rw, e, reinterpret_cast<hipStream_t>(stream)));
    return SCG_OK;
}

// H is the weighted A of SPEC §22.1 at the order's phi, grad the unweighted b of §16.1 / §18.2 for yv = e: gram_call's checks, in
// gram_call's sequence, behind the order's
int scg_basis_gram_irls(scg_ctx *c, int32_t order, int64_t n, const float *x, const float *y, const float *vx, const float *vy,
                        const float *rw, const float *e, int32_t n_seg, const int64_t *offsets, float *H, float *grad, void *stream) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_basis_gram_irls: null ctx");
    const int F = basis_order_features(order);
    if (!F) return fail(c, SCG_ERR_INVALID, "scg_basis_gram_irls: order must be 3, 5 or 7");
    GramArgs G = {{{x, y, vx, vy}, {x, y, vx, vy}}, e, H, grad};
    G.y_stride = 0; G.n_tgt = 1; G.rw = rw;
    return gram_call(c, "scg_basis_gram_irls", !x || !y || !vx || !vy || !rw || !e || !H || !grad || !offsets, false, n, n_seg, offsets,
                     F, G, false, order == 3 ? launch_basis_gram_irls_3 : (order == 5 ? launch_feature_gram_irls : launch_basis_gram_irls_7),
                     stream);
}

int scg_basis_values(scg_ctx *c, int32_t order, int64_t n, const float *x, const float *y, const float *vx, const float *vy,
                     const float *V, int32_t m, float *out, void *stream) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_basis_values: null ctx");
    if (!basis_order_features(order)) return fail(c, SCG_ERR_INVALID, "scg_basis_values: order must be 3, 5 or 7");
    if (n < 0 || !x || !y || !vx || !vy || !V || !out) return fail(c, SCG_ERR_INVALID, "scg_basis_values: bad argument");
    if (m < 1 || m > SCG_BASIS_VALUES_MAX_ROWS) return fail(c, SCG_ERR_INVALID, "scg_basis_values: m out of range [1, SCG_BASIS_VALUES_MAX_ROWS]");
    SCG_CHECK_ASYNC(c);
    SCG_ON_DEVICE(c, "scg_basis_values");
    if (n == 0) return SCG_OK;
    const float *st[4] = {x, y, vx, vy};
    SCG_HIP(c, launch_basis_values(order, n, st, V, m, out, reinterpret_cast<hipStream_t>(stream)));
    return SCG_OK;
}

// ---- SPEC §27: the instruments of the lambda-return targets
int scg_row_values(scg_ctx *c, int64_t n, const float *x, const float *y, const float *vx, const float *vy, const uint8_t *tab,
                   const float *W, int32_t n_tab, float *v, uint8_t *a, void *stream) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_row_values: null ctx");
    if (n < 0) return fail(c, SCG_ERR_INVALID, "scg_row_values: n must be >= 0");
    if (!x || !y || !vx || !vy || !tab || !W || !v) return fail(c, SCG_ERR_INVALID, "scg_row_values: null array argument");
    if (n_tab < 1 || n_tab > c->n_vf) return fail(c, SCG_ERR_INVALID, "scg_row_values: n_tab out of range [1, n_vf]");
    SCG_CHECK_ASYNC(c);
    SCG_ON_DEVICE(c, "scg_row_values");
    if (n == 0) return SCG_OK;
    const RowValuesArgs A = {x, y, vx, vy, tab, W, v, a, n, n_tab};
    SCG_HIP(c, launch_row_values(A, reinterpret_cast<hipStream_t>(stream)));
    return SCG_OK;
}

int scg_lambda_returns(scg_ctx *c, int32_t n_env, const int64_t *offsets, int64_t total, const float *reward, const uint8_t *done,
                       const uint8_t *vf, const uint8_t *term, const float *v0, const float *vk, double gamma, double lam,
                       double r_option_success, double *y0, double *yk, void *stream) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_lambda_returns: null ctx");
    if (n_env < 0) return fail(c, SCG_ERR_INVALID, "scg_lambda_returns: n_env must be >= 0");
    if (total < 0) return fail(c, SCG_ERR_INVALID, "scg_lambda_returns: total must be >= 0");
    if (!offsets || !reward || !done || !vf || !term || !v0 || !vk || !y0 || !yk)
        return fail(c, SCG_ERR_INVALID, "scg_lambda_returns: null array argument");
    if (!(gamma >= 0.0 && gamma <= 1.0)) return fail(c, SCG_ERR_INVALID, "scg_lambda_returns: gamma must be in [0, 1]");
    if (!(lam >= 0.0 && lam <= 1.0)) return fail(c, SCG_ERR_INVALID, "scg_lambda_returns: lam must be in [0, 1]");
    SCG_CHECK_ASYNC(c);
    SCG_ON_DEVICE(c, "scg_lambda_returns");
    if (n_env == 0 || total == 0) return SCG_OK;
    const LambdaReturnsArgs A = {offsets, reward, done, vf, term, v0, vk, y0, yk, gamma, lam, r_option_success, total, n_env};
    SCG_HIP(c, launch_lambda_returns(A, reinterpret_cast<hipStream_t>(stream)));
    return SCG_OK;
}

// ---- SPEC §28: the scan with a trace coefficient per row
int scg_trace_returns(scg_ctx *c, int32_t n_env, const int64_t *offsets, int64_t total, const float *reward, const uint8_t *done,
                      const uint8_t *vf, const uint8_t *term, const uint8_t *action, const uint8_t *ag, const float *v0, const float *vk,
                      double gamma, const double *lam_vf, int32_t n_lam, uint32_t flags, double r_option_success, double *y0, double *yk,
                      double *h, void *stream) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_trace_returns: null ctx");
    if (n_env < 0) return fail(c, SCG_ERR_INVALID, "scg_trace_returns: n_env must be >= 0");
    if (total < 0) return fail(c, SCG_ERR_INVALID, "scg_trace_returns: total must be >= 0");
    if (!offsets || !reward || !done || !vf || !term || !action || !ag || !v0 || !vk || !lam_vf || !y0 || !yk)
        return fail(c, SCG_ERR_INVALID, "scg_trace_returns: null array argument");
    if (n_lam < 1 || n_lam > c->n_vf) return fail(c, SCG_ERR_INVALID, "scg_trace_returns: n_lam out of range [1, n_vf]");
    if (!(gamma >= 0.0 && gamma <= 1.0)) return fail(c, SCG_ERR_INVALID, "scg_trace_returns: gamma must be in [0, 1]");
    for (int k = 0; k < n_lam; ++k)
        if (!(lam_vf[k] >= 0.0 && lam_vf[k] <= 1.0)) return fail(c, SCG_ERR_INVALID, "scg_trace_returns: lam_vf must be in [0, 1]");
    if (flags & ~SCG_TRACE_CUT) return fail(c, SCG_ERR_INVALID, "scg_trace_returns: unknown flag bits");
    SCG_CHECK_ASYNC(c);
    SCG_ON_DEVICE(c, "scg_trace_returns");
    if (n_env == 0 || total == 0) return SCG_OK;
    TraceReturnsArgs A = {offsets, reward, done, vf, term, action, ag, v0, vk, y0, yk, h, gamma, r_option_success, {}, total, n_env, n_lam,
                          flags};
    for (int k = 0; k < MAX_VF; ++k) A.lam[k] = k < n_lam ? lam_vf[k] : lam_vf[0];
    SCG_HIP(c, launch_trace_returns(A, reinterpret_cast<hipStream_t>(stream)));
    return SCG_OK;
}

// ---- SPEC §29: the cross row values of the double-estimator targets
int scg_row_values_cross(scg_ctx *c, int64_t n, const float *x, const float *y, const float *vx, const float *vy, const uint8_t *tab,
                         const float *W_sel, const float *W_val, int32_t n_tab, const uint8_t *act, uint32_t flags, float *v,
                         uint8_t *a, float *vs, void *stream) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_row_values_cross: null ctx");
    if (n < 0) return fail(c, SCG_ERR_INVALID, "scg_row_values_cross: n must be >= 0");
    const bool given = (flags & SCG_CROSS_GIVEN) != 0;
    if (!x || !y || !vx || !vy || !tab || !W_val || !v || (!given && !W_sel))
        return fail(c, SCG_ERR_INVALID, "scg_row_values_cross: null array argument");
    if (n_tab < 1 || n_tab > c->n_vf) return fail(c, SCG_ERR_INVALID, "scg_row_values_cross: n_tab out of range [1, n_vf]");
    if (flags & ~SCG_CROSS_GIVEN) return fail(c, SCG_ERR_INVALID, "scg_row_values_cross: unknown flag bits");
    if (given && (!act || vs)) return fail(c, SCG_ERR_INVALID, "scg_row_values_cross: SCG_CROSS_GIVEN needs act and takes no vs");
    SCG_CHECK_ASYNC(c);
    SCG_ON_DEVICE(c, "scg_row_values_cross");
    if (n == 0) return SCG_OK;
    const RowValuesCrossArgs A = {x, y, vx, vy, tab, W_sel, W_val, given ? act : nullptr, v, a, vs, n, n_tab};
    SCG_HIP(c, launch_row_values_cross(A, given, reinterpret_cast<hipStream_t>(stream)));
    return SCG_OK;
}

// ---- SPEC §30.1: the device record store
int scg_record_append(scg_ctx *c, const scg_record *launch, const scg_record_store *store, int32_t cap, void *stream) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_record_append: null ctx");
    if (!launch || !store) return fail(c, SCG_ERR_INVALID, "scg_record_append: null launch or store");
    if (!launch->len || !store->have || !store->overflow)
        return fail(c, SCG_ERR_INVALID, "scg_record_append: launch->len, store->have and store->overflow are required");
    if (launch->n < 1) return fail(c, SCG_ERR_INVALID, "scg_record_append: launch->n must be >= 1");
    if (launch->rows < 1) return fail(c, SCG_ERR_INVALID, "scg_record_append: launch->rows must be >= 1");
    if (cap < 1) return fail(c, SCG_ERR_INVALID, "scg_record_append: cap must be >= 1");
    SCG_CHECK_ASYNC(c);
    SCG_ON_DEVICE(c, "scg_record_append");
    const RecordAppendArgs A = {{{launch->x, store->x}, {launch->y, store->y}, {launch->vx, store->vx}, {launch->vy, store->vy},
                                 {launch->reward, store->reward}, {launch->action, store->action}, {launch->done, store->done},
                                 {launch->vf, store->vf}, {launch->term, store->term}, {launch->option_id, store->option_id}},
                                launch->len, store->have, store->overflow, launch->n, launch->rows, cap};
    SCG_HIP(c, launch_record_append(A, reinterpret_cast<hipStream_t>(stream)));
    return SCG_OK;
}

int scg_record_offsets(scg_ctx *c, int32_t n, const int32_t *have, int64_t *offsets, void *stream) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_record_offsets: null ctx");
    if (n < 0) return fail(c, SCG_ERR_INVALID, "scg_record_offsets: n must be >= 0");
    if (!offsets || (n > 0 && !have)) return fail(c, SCG_ERR_INVALID, "scg_record_offsets: null array argument");
    SCG_CHECK_ASYNC(c);
    SCG_ON_DEVICE(c, "scg_record_offsets");
    SCG_HIP(c, launch_record_offsets(n, have, offsets, reinterpret_cast<hipStream_t>(stream)));
    return SCG_OK;
}

int scg_record_pack(scg_ctx *c, int32_t n, int32_t cap, const scg_record_store *store, const int64_t *offsets, int64_t total, float *x,
                    float *y, float *vx, float *vy, float *reward, uint8_t *action, uint8_t *done, uint8_t *vf, uint8_t *term,
                    int8_t *option_id, int32_t *env, int32_t *row, uint8_t *tab0, uint8_t *tabk, uint8_t *tabA, void *stream) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_record_pack: null ctx");
    if (n < 0) return fail(c, SCG_ERR_INVALID, "scg_record_pack: n must be >= 0");
    if (cap < 1) return fail(c, SCG_ERR_INVALID, "scg_record_pack: cap must be >= 1");
    if (total < 0) return fail(c, SCG_ERR_INVALID, "scg_record_pack: total must be >= 0");
    if (!store || !offsets) return fail(c, SCG_ERR_INVALID, "scg_record_pack: null store or offsets");
    const RecordPackArgs A = {{{store->x, x}, {store->y, y}, {store->vx, vx}, {store->vy, vy}, {store->reward, reward},
                               {store->action, action}, {store->done, done}, {store->vf, vf}, {store->term, term},
                               {store->option_id, option_id}},
                              store->done, store->vf, store->term, offsets, env, row, tab0, tabk, tabA, total, n, cap};
    for (int k = 0; k < RS_FIELDS; ++k)
        if (A.f[k].dst && !A.f[k].src) return fail(c, SCG_ERR_INVALID, "scg_record_pack: a flat array of a field the store does not keep");
    if ((tab0 || tabk || tabA) && (!store->done || !store->vf || !store->term))
        return fail(c, SCG_ERR_INVALID, "scg_record_pack: the tables need the store's done, vf and term");
    SCG_CHECK_ASYNC(c);
    SCG_ON_DEVICE(c, "scg_record_pack");
    if (n == 0 || total == 0) return SCG_OK;
    SCG_HIP(c, launch_record_pack(A, reinterpret_cast<hipStream_t>(stream)));
    return SCG_OK;
}

// ---- SPEC §31: the pinned-order ridge solve
int scg_ridge_solve(scg_ctx *c, int32_t F, int32_t n_mat, int32_t n_rhs, const float *A, const float *B, const double *lam,
                    const double *mu, const uint8_t *skip, double *work, double *Delta, int32_t *info, void *stream) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_ridge_solve: null ctx");
    if (F < RIDGE_TILE || F > SCG_RIDGE_MAX_F || F % RIDGE_TILE != 0)
        return fail(c, SCG_ERR_INVALID, "scg_ridge_solve: F must be a positive multiple of 16 up to SCG_RIDGE_MAX_F");
    if (n_mat < 1 || n_mat > SCG_GRAM_MAX_SEGMENTS) return fail(c, SCG_ERR_INVALID, "scg_ridge_solve: n_mat out of range [1, SCG_GRAM_MAX_SEGMENTS]");
    if (n_rhs < 1 || n_rhs > SCG_GRAM_MAX_TARGETS) return fail(c, SCG_ERR_INVALID, "scg_ridge_solve: n_rhs out of range [1, SCG_GRAM_MAX_TARGETS]");
    if (!A || !B || !lam || !mu || !skip || !work || !Delta || !info) return fail(c, SCG_ERR_INVALID, "scg_ridge_solve: null array argument");
    SCG_CHECK_ASYNC(c);
    SCG_ON_DEVICE(c, "scg_ridge_solve");
    RidgeArgs P = {A, B, lam, work, Delta, info, {}, 0, F, n_mat, n_rhs, 0};
    for (int g = 0; g < n_mat; ++g) {
        P.mu[g] = mu[g];
        if (skip[g]) P.skip |= 1ull << g;
    }
    SCG_HIP(c, launch_ridge_solve(P, reinterpret_cast<hipStream_t>(stream)));
    return SCG_OK;
}

int scg_q_values(scg_ctx *c, int32_t n, const float *x, const float *y, const float *vx, const float *vy,
                 const float *Wk, float *q, void *stream) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_q_values: null ctx");
    if (n < 0 || !x || !y || !vx || !vy || !Wk || !q) return fail(c, SCG_ERR_INVALID, "scg_q_values: bad argument");
    SCG_CHECK_ASYNC(c);
    SCG_ON_DEVICE(c, "scg_q_values");
    if (n == 0) return SCG_OK;
    StepArgs A;
    fill_common(c, A);
    A.x = const_cast<float *>(x); A.y = const_cast<float *>(y);
    A.vx = const_cast<float *>(vx); A.vy = const_cast<float *>(vy);
    A.qcache = q; A.W = Wk; A.n = n; A.k_lo = 0; A.k_hi = 0; A.cnts = nullptr; A.learn = 0;
    hipLaunchKernelGGL(td_kernel<MODE_QVAL>, dim3((n + BLOCK_ENVS - 1) / BLOCK_ENVS), dim3(THREADS), 0,
                       reinterpret_cast<hipStream_t>(stream), A);
    SCG_HIP(c, hipGetLastError());
    return SCG_OK;
}

int scg_q_update(scg_ctx *c, int32_t n, int32_t k, const float *x, const float *y, const float *vx,
                 const float *vy, const uint8_t *action, const float *r, const float *cont, const float *xn,
                 const float *yn, const float *vxn, const float *vyn, float *W, uint32_t flags, void *stream) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_q_update: null ctx");
    if (!c->have_map) return fail(c, SCG_ERR_STATE, "scg_q_update: scg_set_map has not been called (scale table)");
    if (n < 0 || n > c->cfg.n_envs) return fail(c, SCG_ERR_INVALID, "scg_q_update: n must be in [0, n_envs]");
    if (k < 0 || k >= c->n_vf) return fail(c, SCG_ERR_INVALID, "scg_q_update: VF index out of range");
    if (!x || !y || !vx || !vy || !action || !r || !cont || !xn || !yn || !vxn || !vyn || !W)
        return fail(c, SCG_ERR_INVALID, "scg_q_update: null array argument");
    SCG_CHECK_ASYNC(c);
    SCG_ON_DEVICE(c, "scg_q_update");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int nblk = (n + BLOCK_ENVS - 1) / BLOCK_ENVS;
    SCG_HIP(c, hipMemsetAsync(c->d_cnts, 0, (size_t)c->nblk * c->n_vf * sizeof(int32_t), s));
    if (n > 0) {
        StepArgs A;
        fill_common(c, A);
        A.x = const_cast<float *>(x); A.y = const_cast<float *>(y);
        A.vx = const_cast<float *>(vx); A.vy = const_cast<float *>(vy);
        A.action = const_cast<uint8_t *>(action); A.reward = const_cast<float *>(r); A.cont_in = cont;
        A.xn = xn; A.yn = yn; A.vxn = vxn; A.vyn = vyn;
        A.W = W; A.n = n; A.k_lo = k; A.k_hi = k; A.learn = 1;
        hipLaunchKernelGGL(td_kernel<MODE_TRANS>, dim3(nblk), dim3(THREADS), 0, s, A);
        SCG_HIP(c, hipGetLastError());
    }
    return launch_reduce(c, W, (flags & SCG_STEP_APPLY) ? 1u : 0u, nblk, s, REDUCE_ONLY);
}

int scg_classifier_predict(scg_ctx *c, int32_t n, const float *x, const float *y, const float *w8, uint8_t *out,
                           void *stream) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_classifier_predict: null ctx");
    if (n < 0 || !x || !y || !w8 || !out) return fail(c, SCG_ERR_INVALID, "scg_classifier_predict: bad argument");
    SCG_CHECK_ASYNC(c);
    SCG_ON_DEVICE(c, "scg_classifier_predict");
    if (n == 0) return SCG_OK;
    hipLaunchKernelGGL(predict_kernel, dim3((n + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       n, x, y, w8, out);
    SCG_HIP(c, hipGetLastError());
    return SCG_OK;
}

// SPEC §24.2: predict_kernel's clf_z before the comparison (the kernel: scg_basis_kernels.hpp); scg_classifier_predict's checks in its sequence
int scg_classifier_logits(scg_ctx *c, int32_t n, const float *x, const float *y, const float *w8, float *z, void *stream) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_classifier_logits: null ctx");
    if (n < 0 || !x || !y || !w8 || !z) return fail(c, SCG_ERR_INVALID, "scg_classifier_logits: bad argument");
    SCG_CHECK_ASYNC(c);
    SCG_ON_DEVICE(c, "scg_classifier_logits");
    if (n == 0) return SCG_OK;
    SCG_HIP(c, launch_classifier_logits(n, x, y, w8, z, reinterpret_cast<hipStream_t>(stream)));
    return SCG_OK;
}

int scg_fit_initiation(scg_ctx *c, int32_t n_fit, const float *xy, const uint8_t *label, const int32_t *offsets,
                       float *w, int32_t iters, float lr, float l2, void *stream) {
    if (!c) return fail(nullptr, SCG_ERR_INVALID, "scg_fit_initiation: null ctx");
    if (n_fit < 0 || iters < 0 || !xy || !label || !offsets || !w)
        return fail(c, SCG_ERR_INVALID, "scg_fit_initiation: bad argument");
    SCG_CHECK_ASYNC(c);
    SCG_ON_DEVICE(c, "scg_fit_initiation");
    if (n_fit == 0 || iters == 0) return SCG_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    for (int q0 = 0; q0 < n_fit; q0 += FIT_BATCH) {        // FIT_G workgroups per option, at most 64 in flight: co-resident
        const int nb = n_fit - q0 < FIT_BATCH ? n_fit - q0 : FIT_BATCH;
        SCG_HIP(c, hipMemsetAsync(c->d_fit_part, 0, (size_t)FIT_BATCH * 2 * FIT_G * 8 * sizeof(unsigned long long), s));   // tags of a past call
        hipLaunchKernelGGL(fit_kernel, dim3(FIT_G, nb), dim3(FIT_T), 0, s, xy, label, offsets, w, iters, lr, l2, q0,
                           c->d_fit_part, (unsigned long long)(c->fit_timeout_s * 1e8), c->d_async);
        SCG_HIP(c, hipGetLastError());
    }
    return SCG_OK;
}

}  // extern "C"
