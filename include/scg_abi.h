/*
 * scg_abi.h — C-ABI of libscg_hip.so, the MI355X (gfx950) hot path of vectorized skill chaining.
 *
 * Reference interface replaced: BASELINE.json's north_star names PinballDomain.step,
 * FourierBasis.features, Option.{policy,beta,initiation_classifier} and SkillChainingAgent.q_update,
 * but the reference at /root/reference is README.md:1-2 only (title + one sentence naming Konidaris &
 * Barto 2009) — it has no code, hence no FFI to bind and no file:line to cite for any entry point
 * (SURVEY.md §0, §8a/b). The signatures below are therefore this build's own; each comment names the
 * north_star symbol the entry point stands in for and the SPEC.md section that defines its arithmetic.
 *
 * Conventions
 *  - plain C, no torch types. All array arguments are DEVICE pointers owned by the caller (e.g.
 *    torch.Tensor.data_ptr()) unless marked HOST. `stream` is a hipStream_t passed as void*
 *    (NULL = default stream). Launches are asynchronous on `stream`; nothing here synchronises.
 *  - every function returns 0 on success or a negative scg_status; scg_last_error(ctx) gives text.
 *    No exceptions cross the boundary.
 *  - one ctx per (device, stream of use); calls on one ctx are not re-entrant. The library owns only
 *    the ctx: map tables, the per-block partial-gradient slabs and the reduced gradient.
 *  - state is SoA: x[N], y[N], vx[N], vy[N] float32.
 */
#ifndef SCG_ABI_H
#define SCG_ABI_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCG_ABI_VERSION 5          /* 2: SCG_ASYNC_STEP_HANDOFF, announced-trigger pointer check, 256-env blocks; 3: scg_apply_update_slots;
                                      4: a second update rule (SCG_STEP_CACHED_QSA + a baseline cache); 5: that rule and its two entry
                                      points are gone again (its definition depended on the launch geometry and it was never the
                                      default), SPEC §4.2's exit rule (an option that ends bootstraps from the root) */
#define SCG_NUM_ACTIONS 5
#define SCG_FOURIER_ORDER 5
#define SCG_NUM_FEATURES 1296      /* (order+1)^4 */
#define SCG_MAX_OPTIONS 5
#define SCG_MAX_EDGES 256
#define SCG_CLF_STRIDE 8           /* floats per classifier row (6 used) */

typedef enum {
    SCG_OK = 0,
    SCG_ERR_INVALID = -1,      /* bad argument / unsupported configuration */
    SCG_ERR_NO_DEVICE = -2,    /* no HIP device / wrong architecture */
    SCG_ERR_HIP = -3,          /* a HIP runtime call failed */
    SCG_ERR_STATE = -4,        /* call order (e.g. step before set_map) */
    SCG_ERR_ASYNC = -5         /* a kernel launched earlier gave up on the device (sticky; see "asynchronous failures") */
} scg_status;

typedef struct scg_ctx scg_ctx;

typedef struct {
    int32_t n_envs;              /* envs on this rank */
    int32_t n_options;           /* chained options 1..n_options (<= SCG_MAX_OPTIONS); VF 0 = root */
    int32_t fourier_order;       /* must be SCG_FOURIER_ORDER */
    int32_t device;              /* HIP device ordinal */
    int64_t env_id_base;         /* global id of local env 0 (SPEC §2) */
    uint64_t seed;
    float gamma, alpha, epsilon, r_option_success;
    int32_t max_episode_steps, max_option_steps;
    int32_t update_count_floor;   /* SPEC §5 apply: the divisor of a value function's summed update is max(n_k, floor). 0 = plain n_k. A value
                                   * function with a handful of update items otherwise takes full-size steps on their average and runs away
                                   * (profiles/r05_oracle_chain_curves_gated.txt: NaN weights in an option few envs run); n_envs / 16 is a safe choice */
    int32_t reoffer_period;       /* SPEC §4.2: an env that stays out of option k although inside its initiation set (option_id = -k) is offered k
                                   * again when (t + global env id) % reoffer_period == 0. A power of two; 1 (or 0) = every step */
} scg_config;

/* flags for scg_step */
#define SCG_STEP_LEARN 1u        /* accumulate the TD gradient (otherwise act + physics + qcache only) */
#define SCG_STEP_APPLY 2u        /* apply it to W in the same call (single-rank path) */
#define SCG_STEP_INTERRUPT 4u    /* SPEC §12, with SCG_STEP_LEARN only: an option that would go on is interrupted when max_a Q_o(s_next, a) <
                                  * max_a Q_0(s_next, a); its update item then bootstraps from the root's max, and the env runs the root next
                                  * (option_id -c or 0, opt_steps 0, qcache = Q_0(s_next, .)). Without SCG_STEP_LEARN: SCG_ERR_INVALID, nothing
                                  * is launched (acting-only interruption is scg_rollout_interrupt) */

int scg_abi_version(void);
int scg_block_envs(void);            /* SPEC §5 block size this library was built with (one 16-wavefront workgroup per block): 256 for libscg_hip.so;
                                        libscg_hip_b128.so / _b64.so are the same source built for 128 / 64 (small env counts). The block size
                                        orders the partial sums of G: a sharded run uses ONE geometry on all ranks */
const char *scg_strerror(int status);
const char *scg_last_error(const scg_ctx *ctx);

int scg_create(scg_ctx **out, const scg_config *cfg);
int scg_destroy(scg_ctx *ctx);
/* change hyper-parameters between steps (n_envs / n_options / device are fixed at create). Validated before anything is assigned:
 * a refused call (SCG_ERR_INVALID: update_count_floor < 0, reoffer_period negative or no power of two; the same two checks as
 * scg_create) changes nothing, and every field of an accepted one holds from the next launch of any entry point on.
 * Domains the fields are defined on: gamma in [0, 1], alpha >= 0, epsilon in [0, 1], r_option_success any finite value,
 * max_episode_steps >= 1, max_option_steps >= 1, update_count_floor >= 0, reoffer_period 0 or a power of two up to 2^30 (values
 * outside the first six are not validated and have no defined meaning). */
int scg_set_hparams(scg_ctx *ctx, float gamma, float alpha, float epsilon, float r_option_success,
                    int32_t max_episode_steps, int32_t max_option_steps, int32_t update_count_floor, int32_t reoffer_period);

/* SPEC §1.1. All HOST pointers, copied. edges[n_edges][8], starts[n_starts][2], scale[1296].
 * map_scalars = {R, hstep, R2, TX, TY, TR2}. May be called again between steps: the next launch then sees the new map only
 * (edge count, start list and its length, cell masks); the env states are the caller's and must be valid for it. */
int scg_set_map(scg_ctx *ctx, const float *edges, int32_t n_edges, const float *starts, int32_t n_starts,
                const float map_scalars[6], const float *scale);

/* The fused step-batch: Option.policy (act from qcache) -> PinballDomain.step -> reset/bookkeeping ->
 * Option.beta / option selection -> FourierBasis.features -> Q -> SkillChainingAgent.q_update
 * (SPEC §1.3-§5). In/out: x,y,vx,vy, option_id, opt_steps, ep_steps, qcache[5][N].
 * Out: action[N] u8, reward[N] f32, done[N] u8 (0 live, 1 goal, 2 time-limit).
 * W[n_vf][5][1296] (updated iff SCG_STEP_APPLY), clf[n_vf][8] (row 0 unused), enabled bit k = option k.
 * t = step counter (RNG key). */
int scg_step(scg_ctx *ctx, float *x, float *y, float *vx, float *vy, int32_t *option_id,
             int32_t *opt_steps, int32_t *ep_steps, float *qcache, uint8_t *action, float *reward,
             uint8_t *done, float *W, const float *clf, uint32_t enabled_mask, uint64_t t,
             uint32_t flags, void *stream);

/* scg_step under a gate table (SPEC §26.1). `gate` is a DEVICE array [n_vf][2][5][1296] in SPEC §25's layout: row [k][0] the option
 * side, [k][1] the root side, row 0 never read. Bit k of gate_mask (1 <= k <= n_options): an env about to enter option k does so iff
 * max_a Q(s_next, a) under gate[k][0] >= the same under gate[k][1] (SPEC §3.1's evaluation order, §5's max order; a NaN on either side
 * declines). An option whose bit is clear keeps §4.2's comparison on this step's W. Nothing else differs from scg_step: an entered env's
 * qcache is Q_k(s_next, .) under W, a declined one's Q_0(s_next, .) with option_id = -k; actions, events, ring, gestation counts, G, n_k
 * and the applied W are scg_step's by bits, and the env order prepared by a learning step is that of the ids it leaves.
 * gate_mask == 0 is scg_step (gate is not read; the same launches). Otherwise one small launch runs between the step kernel and the
 * reduce / commit launch; `gate` is never written, the launch waits for no other workgroup and raises no asynchronous failure bit.
 * Errors: scg_step's, in its sequence; behind them SCG_ERR_INVALID (nothing launched, nothing written), in this order:
 * gate_mask != 0 with gate == NULL; gate_mask with bit 0 or a bit >= n_vf; gate_mask != 0 with SCG_STEP_INTERRUPT; gate_mask != 0 with
 * the diagnostic flag 0x100. */
int scg_step_gated(scg_ctx *ctx, float *x, float *y, float *vx, float *vy, int32_t *option_id,
                   int32_t *opt_steps, int32_t *ep_steps, float *qcache, uint8_t *action, float *reward,
                   uint8_t *done, float *W, const float *clf, uint32_t enabled_mask, uint64_t t,
                   uint32_t flags, void *stream, const float *gate, uint32_t gate_mask);

/* ---- acting rollouts (SPEC §8): K acting steps in ONE launch, no learning ----
 * scg_rollout advances the envs n_steps times from t0 exactly as n_steps calls of scg_step(flags = 0) at t = t0 .. t0+n_steps-1
 * would (state, option_id, opt_steps, ep_steps and qcache after every step; action / reward / done of the last step), bit for
 * bit and whatever the block build. A workgroup owns a fixed range of envs for the whole launch and nothing crosses
 * workgroups: the launch cannot hang and raises no asynchronous failure bit. It never writes the trace buffers, events,
 * ev_len, gestation success counts, gradient buffers or W, and it does not read or clear an announced collect trigger.
 * Afterwards the ctx's prepared env order is invalid, as after scg_invalidate_order.
 *   SCG_ROLLOUT_BEGIN        every env starts a new episode first, with the RNG at t0 (SPEC §1.4's reset, done forced to 2, then
 *                            §4.2's selection on the start state with o = 0); the n_steps steps then run at t0+1 .. t0+n_steps.
 *                            BEGIN zeroes stats->ep_return and stats->finished. n_steps = 0 is allowed with BEGIN only; such a
 *                            launch leaves action / reward / done untouched
 *   SCG_ROLLOUT_ONE_EPISODE  an env whose stats->finished[e] != 0 at entry is not stepped (none of its arrays is written); a
 *                            step that ends an episode sets finished[e] = 1 (with or without this flag)
 * `stats` (HOST struct of DEVICE pointers, may be NULL; any member may be NULL = not kept): in/out per-env counters, so one
 * evaluation may span several launches (SPEC §8 table). The caller zeroes them; BEGIN zeroes ep_return and finished.
 * SCG_ERR_INVALID: null ctx or array, n_steps outside [0, SCG_ROLLOUT_MAX_STEPS], n_steps == 0 without BEGIN, ONE_EPISODE
 * without stats->finished. SCG_ERR_STATE before scg_set_map. The cap keeps one launch to tens of milliseconds at the largest
 * batch sizes. The launch geometry (envs per wave, 2 .. 32) is picked from N; the environment variable SCG_ROLLOUT_EPW pins it
 * (tests, measurements; results do not depend on it; another value is SCG_ERR_INVALID). */
typedef struct {
    float *ep_return;              /* [N] return of the running episode */
    double *ret_sum;               /* [N] sum of the recorded episodes' returns */
    int32_t *episodes, *goals, *len_sum;        /* [N] episodes recorded, of them ended in the goal, their summed lengths */
    int32_t *vf_steps, *entries, *declines, *successes;   /* [n_vf][N] each: steps run per VF, option entries, value-gate
                                                             declines, option successes */
    uint8_t *finished;             /* [N] an episode has ended since BEGIN */
} scg_rollout_stats;
#define SCG_ROLLOUT_BEGIN 1u
#define SCG_ROLLOUT_ONE_EPISODE 2u
#define SCG_ROLLOUT_MAX_STEPS 1024
int scg_rollout(scg_ctx *ctx, float *x, float *y, float *vx, float *vy, int32_t *option_id, int32_t *opt_steps,
                int32_t *ep_steps, float *qcache, uint8_t *action, float *reward, uint8_t *done,
                const float *W, const float *clf, uint32_t enabled_mask, uint64_t t0, int32_t n_steps,
                uint32_t flags, const scg_rollout_stats *stats, void *stream);

/* ---- option trials (SPEC §9): each entry runs one option from a given state until that option terminates ----
 * Entry i (0 <= i < n) runs option k = option[i] from s0 = (x, y, vx, vy)[i]: Q_k(s0, .) first (no physics, no RNG draw), then
 * steps j = 0, 1, ... at t = t0 + j with RNG key (env_id_base + i, t), each bit for bit what scg_step(flags = 0) does for an env
 * with option_id = k, opt_steps = j, ep_steps = j (act, physics, done, SPEC §4.2's termination of k; no selection, value gate,
 * re-offer or reset), until the option terminates: after at most min(max_option_steps, max_episode_steps) steps. W and clf are
 * frozen; parents, the gestation mask and the hyper-parameters are the ctx's; k counts as known when it is in enabled | gest.
 * `out` is a HOST struct of DEVICE pointers, each [n]: outcome is required, any other member may be NULL (not written).
 *   outcome  0 not run (k outside 1..n_options or not known: no other output of the entry is written), else the reason the
 *            terminating step ended the option, first match wins: SUCCESS (target reached), EPISODE_END (done != 0),
 *            LEFT_INITIATION (s' outside I_k), TIMEOUT (max_option_steps)
 *   steps    steps taken (>= 1);  ret  sequential binary32 sum of r_o = reward + (succ ? r_option_success : 0)
 *   disc_ret sum of gamma^j r_o (g = 1, d = 0; per step d = d + g r_o, g = g gamma, each product and sum rounded, no fma)
 *   v0       max_a Q_k(s0, a) (SPEC §5's max order);  end_x/y/vx/vy  s' of the terminating step (after the physics)
 * n is any value >= 1, unrelated to cfg.n_envs. Results do not depend on the launch geometry (SCG_ROLLOUT_EPW pins it, as for
 * scg_rollout) or the block build. A trial writes nothing else: no env arrays, trace buffers, events, gestation counts, gradient
 * buffers or W; an announced collect trigger and the prepared env order are left alone. No asynchronous failure bit is raised.
 * SCG_ERR_INVALID: null ctx, array, out or out->outcome; n < 1; min(max_option_steps, max_episode_steps) > SCG_TRIAL_MAX_STEPS.
 * SCG_ERR_STATE before scg_set_map. */
typedef struct {
    uint8_t *outcome;
    int32_t *steps;
    float *ret, *disc_ret, *v0, *end_x, *end_y, *end_vx, *end_vy;
} scg_trial_out;
#define SCG_TRIAL_SUCCESS 1u
#define SCG_TRIAL_EPISODE_END 2u
#define SCG_TRIAL_LEFT_INITIATION 3u
#define SCG_TRIAL_TIMEOUT 4u
#define SCG_TRIAL_MAX_STEPS SCG_ROLLOUT_MAX_STEPS
int scg_option_trials(scg_ctx *ctx, int32_t n, const float *x, const float *y, const float *vx, const float *vy,
                      const int32_t *option, const float *W, const float *clf, uint32_t enabled_mask, uint64_t t0,
                      const scg_trial_out *out, void *stream);

/* ---- recorded rollouts and trials (SPEC §10): the per-step rows of a window of envs / entries ----
 * scg_rollout_record and scg_option_trials_record are scg_rollout and scg_option_trials plus a record `rec` (HOST struct of
 * DEVICE pointers). Recording changes nothing else: every output and counter of the launch is bit for bit the same as without.
 * The record covers envs (rollout) or entries (trials) first .. first+n-1, rows rows each; every field is a [rows][n] array,
 * element (j, r) at j * n + r with r = e - first. Row j is pseudo-step j of the launch:
 *   x, y, vx, vy  s' (the state after the step's physics, before SPEC §1.4's reset; the begin row: the episode's start state)
 *   action (255 on the begin row), reward, done (SPEC §1.4; 2 on the begin row)
 *   vf        o, the value function that ran the step (the option id at entry, out-of-range and negative ids giving 0)
 *   option_id the id the step writes (after the selection and the value gate)
 *   term      0 while the option goes on or for o = 0, else the SCG_TRIAL_* code of the step (first match wins)
 * len[r] (required) is the number of rows written, always a prefix: every pseudo-step, or with ONE_EPISODE up to and including
 * the step that ended the episode, 0 for an env skipped at entry; for trials min(steps, rows), 0 for an entry not run. Rows at
 * or beyond len are not written; any field but len may be NULL (not recorded). With BEGIN (or BEGIN_AT) row 0 is the begin
 * pseudo-step and the steps fill rows 1 .. n_steps. Trials: vf = option_id = k on every row, and the last row's term is the
 * outcome. rec = NULL is the call without a record.
 *   SCG_ROLLOUT_BEGIN_AT  BEGIN with SPEC §1.4's reset replaced by the caller's state: (x, y, vx, vy)[e] as given (velocities
 *                         kept, not validated), ep_steps = 0, no RNG draw for a start index; then §4.2's selection with o = 0, as
 *                         BEGIN. scg_rollout_record only; not together with BEGIN.
 * SCG_ERR_INVALID, beyond scg_rollout's / scg_option_trials' own: rec without len; rec->n < 1; rec->first < 0; first + n beyond
 * N (cfg.n_envs, or the trials' n); rollout rows < n_steps + (BEGIN or BEGIN_AT); trial rows < 1; BEGIN together with BEGIN_AT. */
typedef struct {
    int32_t first, n, rows;                /* envs / entries first .. first+n-1, rows per env */
    int32_t *len;                          /* [n], required */
    float *x, *y, *vx, *vy, *reward;       /* [rows][n]; any may be NULL = not recorded */
    uint8_t *action, *done, *vf, *term;
    int8_t *option_id;
} scg_record;
#define SCG_ROLLOUT_BEGIN_AT 4u
int scg_rollout_record(scg_ctx *ctx, float *x, float *y, float *vx, float *vy, int32_t *option_id, int32_t *opt_steps,
                       int32_t *ep_steps, float *qcache, uint8_t *action, float *reward, uint8_t *done,
                       const float *W, const float *clf, uint32_t enabled_mask, uint64_t t0, int32_t n_steps,
                       uint32_t flags, const scg_rollout_stats *stats, const scg_record *rec, void *stream);
int scg_option_trials_record(scg_ctx *ctx, int32_t n, const float *x, const float *y, const float *vx, const float *vy,
                             const int32_t *option, const float *W, const float *clf, uint32_t enabled_mask, uint64_t t0,
                             const scg_trial_out *out, const scg_record *rec, void *stream);

/* ---- interrupting rollouts (SPEC §11): §8's rollout with a running option cut short where the root's value is higher ----
 * scg_rollout_interrupt is scg_rollout_record with one change on every step of an env whose option o >= 1 goes on (SPEC §4.2's
 * keep): with V_k = max_a Q_k(s', a) (this launch's W, §5's max order), the step is interrupted unless V_o >= V_0 (ties keep the
 * option, a NaN on either side interrupts). An interrupted step writes option_id = -c, with c the smallest enabled option whose
 * initiation set holds s' and whose target region does not (0 if none: option_id = 0), opt_steps = 0 and qcache = Q_0(s', .):
 * the root runs next and c is offered again on §4.2's re-offer schedule. Nothing else of the step changes (action, physics, done,
 * reset, the §8 counters); the begin pseudo-step never interrupts.
 * `interrupts` (DEVICE [n_vf][N] int32, in/out, may be NULL = not kept): interrupts[o][e] += 1 per interrupted step.
 * `rec` (may be NULL) as for scg_rollout_record; an interrupted row has vf = o, the option_id written, term =
 * SCG_ROLLOUT_TERM_INTERRUPTED (never together with another code: an interrupt needs keep). Flags BEGIN, ONE_EPISODE and
 * BEGIN_AT, validated as for scg_rollout_record, with the same errors. Results do not depend on the launch geometry or the block
 * build. scg_rollout and scg_rollout_record never interrupt. */
#define SCG_ROLLOUT_TERM_INTERRUPTED 5u
int scg_rollout_interrupt(scg_ctx *ctx, float *x, float *y, float *vx, float *vy, int32_t *option_id, int32_t *opt_steps,
                          int32_t *ep_steps, float *qcache, uint8_t *action, float *reward, uint8_t *done,
                          const float *W, const float *clf, uint32_t enabled_mask, uint64_t t0, int32_t n_steps,
                          uint32_t flags, const scg_rollout_stats *stats, int32_t *interrupts, const scg_record *rec,
                          void *stream);

/* ---- rollouts with a selection rule (SPEC §14): which of several candidate options an env is offered ----
 * scg_rollout_select is scg_rollout_interrupt plus `rules` and `overrides`. rules = 0 is scg_rollout_record and rules =
 * SCG_SELECT_INTERRUPT is scg_rollout_interrupt (the same kernels, the same results). With SCG_SELECT_BEST an env that is offered an
 * option is offered the candidate of the highest value instead of the lowest-numbered one: with C = {k : enabled, s_next in k's
 * initiation set and outside its target region} and V_k = max_a Q_k(s_next, a) (this launch's W, §5's max order), c* = the k in C
 * with the largest V_k (ties: the lowest k; a NaN never wins; all NaN: min C), and §4.2's gate is applied to c*: option_id = c* if
 * V_c* >= V_0, else -c* with qcache = Q_0. An env that stayed out of any member of C (option_id = -k, k in C) is offered again only on
 * §4.2's re-offer schedule and keeps its option_id in between. Where C has at most one member every output equals rules without
 * BEST, bit for bit. Together with SCG_SELECT_INTERRUPT, §11 is unchanged (an interrupted step writes -min C).
 * `overrides` (DEVICE [n_vf][N] int32, in/out, may be NULL): overrides[c*][e] += 1 when env e enters c* != min C; never written
 * without SCG_SELECT_BEST. `interrupts` is written with SCG_SELECT_INTERRUPT only. Flags, `rec`, the write set and the errors are
 * scg_rollout_record's; SCG_ERR_INVALID also for an unknown bit in `rules` (nothing is launched). Results do not depend on the
 * launch geometry or the block build; the kernel talks to no other workgroup, so it raises no asynchronous failure bit. */
#define SCG_SELECT_INTERRUPT 1u   /* SPEC §11 */
#define SCG_SELECT_BEST      2u   /* SPEC §14 */
int scg_rollout_select(scg_ctx *ctx, float *x, float *y, float *vx, float *vy, int32_t *option_id, int32_t *opt_steps,
                       int32_t *ep_steps, float *qcache, uint8_t *action, float *reward, uint8_t *done,
                       const float *W, const float *clf, uint32_t enabled_mask, uint64_t t0, int32_t n_steps,
                       uint32_t flags, const scg_rollout_stats *stats, int32_t *interrupts, int32_t *overrides,
                       const scg_record *rec, uint32_t rules, void *stream);

/* ---- audited rollouts (SPEC §15): a forced first choice and the discounted TASK return, to check the value gate against ----
 * scg_rollout_audit is scg_rollout_select (any `rules`) plus `audit`, a HOST struct of DEVICE pointers, each [N], any may be NULL.
 * audit = NULL, or every member NULL, is scg_rollout_select: the same kernels, the same results.
 * The begin pseudo-step (BEGIN or BEGIN_AT) only: with C the candidate set of the start state s0 (scg_rollout_select's C, for every
 * `rules`) and f = force[e]: f = +k, k in C: env e is offered k and enters it whatever the gate says (option_id = k, qcache =
 * Q_k(s0, .); entries[k] += 1; with SCG_SELECT_BEST overrides[k] += 1 when k != min C). f = -k, k in C: env e is offered k and declines
 * it (option_id = -k, qcache = Q_0(s0, .); declines[k] += 1; k is offered again on §4.2's re-offer schedule). f = 0, |f| outside
 * 1..n_options or |f| not in C (not enabled, gestating, s0 outside its set or inside its target): the unaudited choice. Every later
 * step is scg_rollout_select's.
 *   applied [N] uint8   1 where the force decided the begin choice, else 0           (written at the begin pseudo-step)
 *   cand    [N] int8    the option offered at the begin pseudo-step after the force, 0: none          (likewise)
 *   v_root  [N] float   max_a Q_0(s0, a), this launch's W, §5's max order                             (likewise)
 *   v_cand  [N] float   max_a Q_cand(s0, a); written where cand >= 1 only
 *   disc_ret, disc_g [N] float, in/out: the discounted task return d of the running episode and its discount g. BEGIN / BEGIN_AT
 *           set d = 0, g = 1 (what the arrays hold is not read); every real step does d = d + g * reward, then g = g * gamma, each
 *           product and sum rounded to binary32, no fma; reward is the env's reward (the record's `reward`), gamma the context's.
 *   disc_final [N] float: on a step with done != 0, disc_final[e] = d, then d = 0, g = 1 (the last episode ended in the launch;
 *           not written for an env no episode of which ended).
 * An env skipped under ONE_EPISODE writes none of these. The write set is scg_rollout_select's plus the members given. Errors:
 * scg_rollout_select's, and SCG_ERR_INVALID (nothing launched) for `force` without BEGIN or BEGIN_AT, and for disc_ret without
 * disc_g or the reverse. Results do not depend on the launch geometry or the block build; the kernel talks to no other workgroup,
 * so it raises no asynchronous failure bit. */
typedef struct {
    const int8_t *force;
    uint8_t *applied;
    int8_t *cand;
    float *v_root, *v_cand;
    float *disc_ret, *disc_g, *disc_final;
} scg_audit;
int scg_rollout_audit(scg_ctx *ctx, float *x, float *y, float *vx, float *vy, int32_t *option_id, int32_t *opt_steps,
                      int32_t *ep_steps, float *qcache, uint8_t *action, float *reward, uint8_t *done,
                      const float *W, const float *clf, uint32_t enabled_mask, uint64_t t0, int32_t n_steps,
                      uint32_t flags, const scg_rollout_stats *stats, int32_t *interrupts, int32_t *overrides,
                      const scg_record *rec, uint32_t rules, const scg_audit *audit, void *stream);

/* ---- branch rollouts (SPEC §19): resume a given state with the first action forced ----
 * scg_rollout_branch is scg_rollout_audit (any `rules`; `rec` and `audit` may be NULL) plus `first_action`, a DEVICE array [N] of
 * uint8, read only. first_action = NULL, or every entry >= SCG_NUM_ACTIONS, is scg_rollout_audit: the same kernels, the same results.
 * The forced step is the launch's first real step: the step at t0 without a begin flag, at t0 + 1 with BEGIN or BEGIN_AT (with
 * BEGIN_AT an exploring start: the caller's state, then the forced action). For every env that is stepped, first_action[e] <
 * SCG_NUM_ACTIONS replaces §4.3's choice of that step's action; any other value means not forced (255 is the canonical one). The
 * step's RNG draw is made as ever (draws are keyed by (seed, global env id, t): a force shifts no later draw), and everything else
 * of the step is unchanged: physics, done, §4.2, the record row (its `action` is the forced one), the counters, §15's d and g.
 * Every later step is scg_rollout_audit's. An env skipped under ONE_EPISODE ignores its entry and writes nothing.
 * Errors: scg_rollout_audit's, and SCG_ERR_INVALID (nothing launched) for a non-NULL first_action with n_steps == 0: there is no
 * real step to force. The write set is scg_rollout_audit's; first_action is never written. Results do not depend on the launch
 * geometry or the block build; no asynchronous failure bit is raised. */
int scg_rollout_branch(scg_ctx *ctx, float *x, float *y, float *vx, float *vy, int32_t *option_id, int32_t *opt_steps,
                       int32_t *ep_steps, float *qcache, uint8_t *action, float *reward, uint8_t *done,
                       const float *W, const float *clf, uint32_t enabled_mask, uint64_t t0, int32_t n_steps,
                       uint32_t flags, const scg_rollout_stats *stats, int32_t *interrupts, int32_t *overrides,
                       const scg_record *rec, uint32_t rules, const scg_audit *audit, const uint8_t *first_action,
                       void *stream);

/* ---- population rollouts (SPEC §21): several policies in one launch, on common random numbers ----
 * scg_rollout_population is scg_rollout_branch plus `pop`. pop = NULL is scg_rollout_branch: the same kernels, the same results.
 * With pop the context's N envs are C = n_policies ranges of n_per consecutive envs; the envs c * n_per .. (c + 1) * n_per - 1 act
 * under policy c: the weights W[c] (W is then a DEVICE array [C][n_vf][5][1296]), the exploration rate epsilon[c] and the enabled
 * mask enabled[c]. Classifiers, gestation, parents, map and hyper-parameters are the context's for every policy. The draws of env
 * c * n_per + i are those of global env id env_id_base + i for every c (§4.2's re-offer schedule likewise): the policies see the
 * same start states and the same draws. Every array is indexed by the env's position among the N as ever.
 * The contract: for every c the outputs of range c equal BY BITS what scg_rollout_branch writes on a context of n_per envs with the
 * same seed, env_id_base, map, hyper-parameters, classifiers, t0, n_steps, flags and rules, with W[c], epsilon[c], enabled[c], and
 * that range of every input (a record window clipped to the range).
 * Errors: scg_rollout_branch's, in its sequence; after them SCG_ERR_INVALID (nothing launched, nothing written), in this order:
 * n_policies outside [1, SCG_POP_MAX]; n_per < 1; n_policies * n_per != the context's n_envs. The write set is
 * scg_rollout_branch's; W, epsilon and enabled are never written. Results do not depend on the launch geometry or the block
 * build; no asynchronous failure bit is raised. */
#define SCG_POP_MAX 64
typedef struct {            /* HOST struct of DEVICE pointers */
    int32_t n_policies;     /* C in [1, SCG_POP_MAX] */
    int32_t n_per;          /* envs per policy, >= 1; C * n_per == cfg.n_envs */
    const float *epsilon;   /* [C], or NULL: cfg's epsilon for every policy */
    const uint32_t *enabled;/* [C], or NULL: the enabled_mask argument for every policy */
} scg_population;
int scg_rollout_population(scg_ctx *ctx, float *x, float *y, float *vx, float *vy, int32_t *option_id, int32_t *opt_steps,
                           int32_t *ep_steps, float *qcache, uint8_t *action, float *reward, uint8_t *done,
                           const float *W, const float *clf, uint32_t enabled_mask, uint64_t t0, int32_t n_steps,
                           uint32_t flags, const scg_rollout_stats *stats, int32_t *interrupts, int32_t *overrides,
                           const scg_record *rec, uint32_t rules, const scg_audit *audit, const uint8_t *first_action,
                           void *stream, const scg_population *pop);

/* ---- population rollouts with a classifier table per policy (SPEC §24.1) ----
 * scg_rollout_population_clf is scg_rollout_population plus `pop_clf` (scg_population itself is unchanged: callers compiled against
 * it keep working). pop_clf = NULL is scg_rollout_population, which forwards here: the same kernels, the same results.
 * With pop_clf, a DEVICE array [C][n_vf][SCG_CLF_STRIDE], the envs of policy c use the rows pop_clf[c] wherever the rollout reads a
 * classifier: §4.2's membership masks of s' and s_next and all that follows from them (keep / success / left-initiation, the
 * candidate set, the selection, §14's choice, §15's force check, §9's term code in the record). `clf` is then no policy's (as
 * cfg's epsilon is no policy's with pop->epsilon) but is checked as before. Gestation, parents, map and hyper-parameters stay the
 * context's.
 * The contract is scg_rollout_population's with clf = pop_clf[c] on the n_per-env context of range c.
 * Errors: scg_rollout_population's, in its sequence; after them SCG_ERR_INVALID (nothing launched, nothing written) for a
 * non-NULL pop_clf with pop == NULL. The write set is scg_rollout_population's; pop_clf is never written. Results do not depend on
 * the launch geometry or the block build; no asynchronous failure bit is raised. */
int scg_rollout_population_clf(scg_ctx *ctx, float *x, float *y, float *vx, float *vy, int32_t *option_id, int32_t *opt_steps,
                               int32_t *ep_steps, float *qcache, uint8_t *action, float *reward, uint8_t *done,
                               const float *W, const float *clf, uint32_t enabled_mask, uint64_t t0, int32_t n_steps,
                               uint32_t flags, const scg_rollout_stats *stats, int32_t *interrupts, int32_t *overrides,
                               const scg_record *rec, uint32_t rules, const scg_audit *audit, const uint8_t *first_action,
                               void *stream, const scg_population *pop, const float *pop_clf);

/* ---- population rollouts with a gate table per policy (SPEC §25.1) ----
 * scg_rollout_population_gate is scg_rollout_population_clf plus `pop_gate`. pop_gate = NULL is scg_rollout_population_clf, which
 * forwards here: the same kernels, the same results.
 * pop_gate is a DEVICE array [C][n_vf][2][5][1296]. For option k >= 1, pop_gate[c][k][0] is the OPTION side and pop_gate[c][k][1]
 * the ROOT side of policy c's value gate for k; row k = 0 is never read. With it §4.2's line reads
 *     declined = entering && !(Vg_opt >= Vg_root),   Vg_opt = max_a Q(s_next, a) under pop_gate[c][cand][0],
 *                                                     Vg_root = the same under pop_gate[c][cand][1],
 * both in §3.1's evaluation order and §5's max order; a NaN side declines. NOTHING else changes: an entered env's qcache is
 * Q_cand(s_next, .) under W[c], a declined env's Q_0(s_next, .) under W[c]; candidate selection, stay / re-offer, keep / success /
 * termination and the actions are as before; §15's force still replaces the gate's result, and §15's begin outputs v_cand / v_root
 * of an offered env, "the values the gate reads", are Vg_opt / Vg_root.
 * The identity: with pop_gate[c][k][0] = W[c][k] and pop_gate[c][k][1] = W[c][0] every output equals scg_rollout_population_clf's by
 * bits.
 * Errors: scg_rollout_population_clf's, in its sequence; after them SCG_ERR_INVALID (nothing launched, nothing written), in this
 * order: a non-NULL pop_gate with pop == NULL; a non-NULL pop_gate with SCG_SELECT_INTERRUPT or SCG_SELECT_BEST in `rules` (a
 * gated interruption and a gated value-ranked choice are out of scope). The write set is scg_rollout_population's; pop_gate is
 * never written. Results do not depend on the launch geometry or the block build; no asynchronous failure bit is raised. */
int scg_rollout_population_gate(scg_ctx *ctx, float *x, float *y, float *vx, float *vy, int32_t *option_id, int32_t *opt_steps,
                                int32_t *ep_steps, float *qcache, uint8_t *action, float *reward, uint8_t *done,
                                const float *W, const float *clf, uint32_t enabled_mask, uint64_t t0, int32_t n_steps,
                                uint32_t flags, const scg_rollout_stats *stats, int32_t *interrupts, int32_t *overrides,
                                const scg_record *rec, uint32_t rules, const scg_audit *audit, const uint8_t *first_action,
                                void *stream, const scg_population *pop, const float *pop_clf, const float *pop_gate);

/* Device pointers of the ctx-owned reduced gradient G[n_vf][5][1296] and counts n_k[n_vf] (int32)
 * left by the last scg_step(LEARN) — the buffers a multi-rank caller all-reduces (SPEC §5). */
int scg_grad_buffers(scg_ctx *ctx, float **G, int32_t **n_k);
/* Make scg_step / scg_q_update leave G and n_k in caller-owned device buffers instead
 * (G[n_vf][5][1296] float32, n_k[n_vf] int32); NULL, NULL restores the ctx-owned ones. */
int scg_set_grad_buffers(scg_ctx *ctx, float *G, int32_t *n_k);
/* Apply (possibly all-reduced) G / n_k to W: W_k += alpha/n_k * scale * G_k (SPEC §5). */
int scg_apply_update(scg_ctx *ctx, float *W, const float *G, const int32_t *n_k, void *stream);
/* The same pair as ONE all-reduce operand: G_packed holds n_vf*6480 floats of G followed by n_vf floats that
 * receive the update counts as floats (exact: they stay far below 2^24), so a sharded run with shared weights
 * sums (G, n_k) over the ranks with a single latency-bound collective per step. NULL restores the ctx-owned
 * buffers. scg_apply_update_packed reads the counts back from the tail. */
int scg_set_grad_buffer_packed(scg_ctx *ctx, float *G_packed);
int scg_apply_update_packed(scg_ctx *ctx, float *W, const float *G_packed, void *stream);
/* The ORDER-PINNED multi-rank sum (ABI 3): `slots` holds the packed operands of n_slots ranks, slot r at
 * slots + r * slot_stride floats (slot_stride >= n_vf*6480 + n_vf) — what an all-gather of every rank's G_packed leaves —
 * and the update is applied from their sum taken IN SLOT ORDER, ((G_0 + G_1) + G_2) + ..., element by element
 * (SPEC §5): the weights are then identical on every rank of a run and reproducible by the oracle for any number of ranks (the rank count, like the block size and the seed, is part of the run's identity).
 * (An all-reduce's order of additions is the library's business: exact for two ranks, to rounding beyond.) */
int scg_apply_update_slots(scg_ctx *ctx, float *W, const float *slots, int32_t n_slots, int64_t slot_stride, void *stream);

/* ---- the peer transport of the order-pinned sum: no collective on the step path ----
 * The ranks of ONE node (processes on one or several GPUs) each own a region of device memory (plain hipMalloc, ctx-owned):
 * an epoch line, a void line and two packed operands (parity 0 / 1). Every rank maps the others' regions through HIP IPC once;
 * per learning step-batch each rank publishes its operand and sums all of them in rank order itself, with the arithmetic of
 * scg_apply_update_slots: the weights are bit for bit those of an all-gather + scg_apply_update_slots.
 *   scg_peer_export          allocate the region (once; later calls return the same handle) and write its
 *                            hipIpcMemHandle_t to handle_out (HOST, 64 bytes)
 *   scg_peer_open            handles = n_ranks x 64 bytes (HOST) in rank order, as every rank's scg_peer_export left them;
 *                            opens each peer region once (a region of this same process is used directly); n_ranks in [1, 8];
 *                            SCG_ERR_STATE before scg_peer_export or when already open. scg_destroy closes the mappings and
 *                            frees the region: destroy only after every rank has finished its last exchange
 *   (step begin)             FOLDED INTO scg_step: while the peers are open, every scg_step(LEARN) leaves its packed operand in
 *                            this rank's buffer of parity e & 1 (e = the ctx's private exchange counter), whatever
 *                            scg_set_grad_buffer* said; SCG_STEP_APPLY is refused then
 *   scg_peer_exchange_apply  after that step, on the same stream: (a) publish — the void flag of exchange e (set when a workgroup
 *                            of the step gave up), a system-scope release, epoch := e + 1; (b) wait — ONE wave polls every rank's
 *                            epoch until >= e + 1 (system-scope loads, s_sleep between them), bounded by scg_set_peer_timeout of
 *                            wall clock: on expiry SCG_ASYNC_PEER_TIMEOUT is raised and W is left untouched; (c) apply — the
 *                            sum of the n_ranks operands of parity e & 1 in rank order, applied as scg_apply_update_slots does;
 *                            if ANY rank voided its step no rank touches W and each raises SCG_ASYNC_STEP_HANDOFF. Then e += 1.
 *                            Launched even while an asynchronous failure is pending (the peers must not be left waiting); the
 *                            pending failure is returned as SCG_ERR_ASYNC after the launches.
 * The counter e is not the step counter t: a checkpoint reload rewinds t, not e. All ranks make one exchange per learning
 * step-batch. Ranks sharing one GPU must keep the sum of their step grids below the chip's 256 workgroups (the waiting wave
 * holds a CU slot); the Python layer checks that. */
int scg_peer_export(scg_ctx *ctx, void *handle_out);
int scg_peer_open(scg_ctx *ctx, int32_t n_ranks, int32_t rank, const void *handles);
int scg_peer_exchange_apply(scg_ctx *ctx, float *W, void *stream);

/* ---- un-fused entry points (same arithmetic; used by the API facade and the parity tests) ---- */

/* PinballDomain.step (SPEC §1.3) with caller-given actions; no reset. goal[n] u8. */
int scg_pinball_step(scg_ctx *ctx, int32_t n, float *x, float *y, float *vx, float *vy,
                     const uint8_t *action, float *reward, uint8_t *goal, void *stream);
/* FourierBasis.features (SPEC §3): phi[n][1296]. */
int scg_fourier_features(scg_ctx *ctx, int32_t n, const float *x, const float *y, const float *vx,
                         const float *vy, float *phi, void *stream);
/* Feature Gram (SPEC §16.1): for each of n_seg segments of the n recorded states — segment g = samples offsets[g] .. offsets[g+1]-1;
 * offsets HOST int64[n_seg+1], non-decreasing, inside [0, n]; empty segments allowed, samples outside every segment ignored —
 *   A[g][1296][1296] = sum_n phi(s_n) phi(s_n)^T   and, with yv[n] / b given (both or neither),   b[g][1296] = sum_n phi(s_n) yv[n]
 * in SPEC §16.1's pinned order: per entry an fma chain over each slab of SCG_GRAM_SLAB consecutive samples of the segment, the slab
 * sums added in order. phi is never materialised (f32 MFMA operands are built from the state). A and b are fully overwritten (an
 * empty segment: +0), A exactly symmetric; the same bits from every block build. Needs no map (no SCG_ERR_STATE before scg_set_map)
 * and writes A and b only: nothing of the training state. SCG_ERR_INVALID, nothing launched: a null x / y / vx / vy / A / offsets,
 * n < 0, n_seg outside [1, SCG_GRAM_MAX_SEGMENTS], offsets that decrease or leave [0, n], yv without b or b without yv. */
#define SCG_GRAM_SLAB 1024
#define SCG_GRAM_MAX_SEGMENTS 64
#ifndef SCG_GRAM_MACRO_TILE
#define SCG_GRAM_MACRO_TILE 96     /* features a side of one workgroup's block of A (not part of the arithmetic: a test's edge list) */
#endif
int scg_feature_gram(scg_ctx *ctx, int64_t n, const float *x, const float *y, const float *vx, const float *vy,
                     const float *yv /* may be NULL */, int32_t n_seg, const int64_t *offsets /* HOST */,
                     float *A, float *b /* NULL iff yv is NULL */, void *stream);
/* Feature Gram with several right-hand sides (SPEC §20.1): scg_feature_gram's A[g][1296][1296] and, for the n_tgt targets per sample
 * Y[n_tgt][n] (target c of sample n at Y[c * n + n]),   B[g][c][1296] = sum_n phi(s_n) Y[c][n],   1 <= n_tgt <= SCG_GRAM_MAX_TARGETS:
 * the targets are the columns of the one MFMA operand that carries scg_feature_gram's yv, so up to 16 right-hand sides cost what one
 * does. A is by bits scg_feature_gram's A and B[g][c] by bits the b[g] it gives for yv = Y[c], for every n_tgt, whether c is
 * computed alone or among 16, and from every block build. A target that holds NaN or +-inf leaves its own B[.][c] unspecified and
 * every other target and A untouched. A and the n_seg * n_tgt * 1296 floats of B are fully overwritten (an empty segment: +0) and
 * nothing else is written; needs no map; raises no asynchronous status. SCG_ERR_INVALID, nothing launched, in this sequence: a null
 * x / y / vx / vy / Y / A / B / offsets, n < 0, n_seg outside [1, SCG_GRAM_MAX_SEGMENTS], offsets that decrease or leave [0, n],
 * n_tgt outside [1, SCG_GRAM_MAX_TARGETS]. */
#define SCG_GRAM_MAX_TARGETS 16
int scg_feature_gram_targets(scg_ctx *ctx, int64_t n, const float *x, const float *y, const float *vx, const float *vy,
                             const float *Y /* [n_tgt][n] */, int32_t n_tgt, int32_t n_seg, const int64_t *offsets /* HOST */,
                             float *A /* [n_seg][1296][1296] */, float *B /* [n_seg][n_tgt][1296] */, void *stream);
/* Weighted feature Gram (SPEC §22.1): scg_feature_gram_targets with a ROOT weight rw[n] per sample on every operand; the least-squares
 * weight is w_n = rw[n]^2, so no square root is taken. With u_f(n) = fl32(rw[n] * phi_f(s_n)) and t_c(n) = fl32(rw[n] * Y[c][n]) — one
 * IEEE binary32 multiply each, round to nearest, subnormals kept, fused with nothing; phi as scg_fourier_features forms it —
 *   A[g][1296][1296] = sum_n u(n) u(n)^T   and   B[g][c][1296] = sum_n u(n) t_c(n),   0 <= n_tgt <= SCG_GRAM_MAX_TARGETS,
 * on SPEC §16.1's chains: P = fma(u_i(n), u_j(n), P) from +0 over each slab of SCG_GRAM_SLAB samples counted from the segment's first
 * sample, the slab sums added in order. A is exactly symmetric. By bits: rw = 1 everywhere gives scg_feature_gram_targets' A and B (and,
 * with n_tgt = 0, scg_feature_gram's A); rw = 2 everywhere 4 A and 4 B where no partial sum is subnormal; a segment whose last m samples
 * have rw = 0 the unweighted result of the segment shortened by m. A zero weight masks no non-finite value (0 * NaN is NaN): a non-finite
 * rw[n] or state leaves the segment's outputs unspecified, a non-finite Y[c][n] its own B[.][c] and nothing else. A and the
 * n_seg * n_tgt * 1296 floats of B are fully overwritten (an empty segment, n = 0: +0) and nothing else is written; needs no map; raises
 * no asynchronous status; the same bits from every block build. SCG_ERR_INVALID, nothing launched, nothing written, in this sequence: a
 * null x / y / vx / vy / rw / A / offsets, n < 0, n_seg outside [1, SCG_GRAM_MAX_SEGMENTS], offsets that decrease or leave [0, n], n_tgt
 * outside [0, SCG_GRAM_MAX_TARGETS], n_tgt = 0 with a Y or a B, n_tgt >= 1 without Y or without B.
 * Not offered weighted: the cross shape (scg_feature_cross_gram), the orders 3 and 7 of this entry point (scg_basis_gram_irls below has
 * the weighted A at every order); nothing of LSTD-Q, of the fit to realised returns or of the learner uses weights. */
int scg_feature_gram_weighted(scg_ctx *ctx, int64_t n, const float *x, const float *y, const float *vx, const float *vy,
                              const float *rw /* [n] root weights */, const float *Y /* [n_tgt][n], NULL iff n_tgt == 0 */,
                              int32_t n_tgt /* 0 .. SCG_GRAM_MAX_TARGETS */, int32_t n_seg, const int64_t *offsets /* HOST */,
                              float *A /* [n_seg][1296][1296] */, float *B /* [n_seg][n_tgt][1296], NULL iff n_tgt == 0 */, void *stream);
/* Cross-feature Gram (SPEC §17.1): for each of n_seg segments (offsets as in scg_feature_gram) of n recorded samples with two states
 * each, s_n = (x, y, vx, vy)[n] and s2_n = (x2, y2, vx2, vy2)[n],
 *   C[g][1296][1296] = sum_n phi(s_n) phi(s2_n)^T   (rows: features of s, columns: features of s2; not symmetric)
 * in scg_feature_gram's pinned order: per entry an fma chain over each slab of SCG_GRAM_SLAB consecutive samples of the segment, the
 * slab sums added in order. C is fully overwritten (an empty segment: +0); C(s, s2) = C(s2, s)^T and C(s, s) = scg_feature_gram's A,
 * both by bits; the same bits from every block build; the s2 arrays may alias the s arrays. Needs no map and writes C only.
 * SCG_ERR_INVALID, nothing launched: a null array argument, n < 0, n_seg outside [1, SCG_GRAM_MAX_SEGMENTS], offsets that decrease or
 * leave [0, n]. */
#ifndef SCG_CROSS_GRAM_MACRO_TILE
#define SCG_CROSS_GRAM_MACRO_TILE 96   /* features a side (rows and columns alike) of one workgroup's block of C: a test's edge list */
#endif
int scg_feature_cross_gram(scg_ctx *ctx, int64_t n, const float *x, const float *y, const float *vx, const float *vy,
                           const float *x2, const float *y2, const float *vx2, const float *vy2,
                           int32_t n_seg, const int64_t *offsets /* HOST */, float *C, void *stream);
/* ---- the basis-order probe (SPEC §18): the Fourier basis of order p in {3, 5, 7}, F = (p + 1)^4 = 256, 1296, 4096 features, feature
 * ((c1 (p+1) + c2) (p+1) + c3) (p+1) + c4, formed by SPEC §3's operations with 6 replaced by p + 1: at order 5 SPEC §3's bits, and
 * a feature with every c <= q < p has, at order p, the bits it has at order q. Reporting instruments: nothing acts or learns at an
 * order other than 5. All three need no map, raise no asynchronous status and write their output only. SCG_ERR_INVALID, nothing
 * launched, nothing written: a null ctx, then an order outside {3, 5, 7}, then the checks each comment names. */
#define SCG_BASIS_VALUES_MAX_ROWS 8
/* phi[n][F] of order p; at order 5 scg_fourier_features' bits (n < 2^31 there). Then: n < 0, a null array. */
int scg_basis_features(scg_ctx *ctx, int32_t order, int64_t n, const float *x, const float *y, const float *vx, const float *vy,
                       float *phi, void *stream);
/* scg_feature_gram with 1296 -> F: A[n_seg][F][F] and b[n_seg][F], the same slabs, chains, symmetry, +0 for an empty segment, and the
 * same checks in the same sequence; at order 5 scg_feature_gram's bits. For q < p, order q's A and b are the sub-block of order p's
 * at the embedded indices, by bits. */
int scg_basis_gram(scg_ctx *ctx, int32_t order, int64_t n, const float *x, const float *y, const float *vx, const float *vy,
                   const float *yv /* may be NULL */, int32_t n_seg, const int64_t *offsets /* HOST */,
                   float *A, float *b /* NULL iff yv is NULL */, void *stream);
/* out[m][n], out[r][n] = sum_f V[r][f] phi_f(s_n) for the m rows of V[m][F], 1 <= m <= SCG_BASIS_VALUES_MAX_ROWS, in SPEC §18.3's pinned
 * order (per c12 = f / (p+1)^2 an fma chain over c34 from +0, those sums added in c12 order from +0): NOT SPEC §3.1's order, also at
 * order 5. Then: n < 0, a null array, m out of range. */
int scg_basis_values(scg_ctx *ctx, int32_t order, int64_t n, const float *x, const float *y, const float *vx, const float *vy,
                     const float *V, int32_t m, float *out, void *stream);
/* ---- the instruments of the Fourier initiation classifier's fit (SPEC §23): logistic regression on the basis of order p by IRLS.
 * Reporting instruments as the probe above: nothing acts or learns with them. Both need no map, raise no asynchronous status and
 * write their outputs only. */
/* Logistic terms (SPEC §23.1). Per sample, from a logit z[n] and a label[n] (u8, non-zero is 1): p = sigmoid(z) by SPEC §6's formula
 * operation by operation (a NaN and every z <= -87 give 0x1.666d0ep-126, z >= 87 gives 1), l = label != 0 ? 1 : 0, e = l - p,
 * q = 1 - p, s = p * q, rw = sqrt(s): one binary32 operation each, fused with nothing, the square root correctly rounded (+0 for
 * s = +0). Outputs p[n], rw[n] and e[n]. SCG_ERR_INVALID, nothing launched, nothing written, in this sequence: a null ctx, n < 0, a
 * null array. n = 0 succeeds and writes nothing. */
int scg_logistic_terms(scg_ctx *ctx, int64_t n, const float *z, const uint8_t *label, float *p, float *rw, float *e, void *stream);
/* IRLS Gram (SPEC §23.2): for the order p in {3, 5, 7}, F = (p + 1)^4, and the segments of scg_feature_gram,
 *   H[g][F][F] = sum_n u(n) u(n)^T,  u_f(n) = fl32(rw[n] * phi_f(s_n))   (scg_feature_gram_weighted's operands at the order's phi)
 *   grad[g][F] = sum_n phi(s_n) e[n]                                      (the UNWEIGHTED phi: scg_basis_gram's b for yv = e)
 * both on SPEC §16.1's chains. By bits: at order 5 H is scg_feature_gram_weighted's A (n_tgt = 0); at every order grad is
 * scg_basis_gram's b for yv = e whatever rw holds, and H does not depend on e; rw = 1 everywhere gives scg_basis_gram's A; order q's H
 * and grad are the sub-block of order p's at the embedded indices (q < p); H is exactly symmetric; the same bits from every block
 * build. A non-finite rw[n] or state leaves the segment's H and grad unspecified, a non-finite e[n] its grad only; a zero weight masks
 * no NaN. H and grad are fully overwritten (an empty segment, n = 0: +0) and nothing else is written. SCG_ERR_INVALID, nothing
 * launched, nothing written, in this sequence: a null ctx, an order outside {3, 5, 7}, a null x / y / vx / vy / rw / e / H / grad /
 * offsets, n < 0, n_seg outside [1, SCG_GRAM_MAX_SEGMENTS], offsets that decrease or leave [0, n]. */
int scg_basis_gram_irls(scg_ctx *ctx, int32_t order, int64_t n, const float *x, const float *y, const float *vx, const float *vy,
                        const float *rw, const float *e, int32_t n_seg, const int64_t *offsets /* HOST */,
                        float *H /* [n_seg][F][F] */, float *grad /* [n_seg][F] */, void *stream);
/* ---- the pinned-order ridge solve (SPEC §31): a batched binary64 Cholesky factor-and-solve of the Gram kernels' output where it lies.
 * For each of n_mat matrices A[g][F][F] (binary32; only i >= j is read, the strict upper triangle may hold anything) with n_rhs
 * right-hand sides B[g][c][F] (binary32), lam[F] (binary64, device) and the host scalars mu[g]:
 *   M_ij = double(A_ij) (i > j),  M_ii = double(A_ii) + mu[g] * lam[i];   M = L L^T;   Delta[g][c] = M^-1 double(B[g][c])
 * every operation binary64 and rounded on its own (no fma), in SPEC §31.1's order: per entry of L the updates in ascending k, the
 * forward substitution ascending, the backward one descending from F - 1; sqrt and / correctly rounded. Nothing depends on the tiling,
 * the grid, the block build or the batch. On return work[g]'s lower triangle holds L (its strict upper triangle is not written),
 * Delta[n_mat][n_rhs][F] the solutions and info[g] (int32, device) 0, or j + 1 where the pivot of column j failed !(t > 0) (a NaN
 * included): then Delta[g] = +0, work[g] holds the block columns of 16 finished before, and the other matrices are unaffected. skip[g] != 0 (HOST
 * u8): Delta[g] = +0, info[g] = 0, A[g], B[g] and work[g] are not touched. A memset of info, F / 16 factor launches and one substitution launch on `stream`; no
 * workgroup waits on another. Needs no map, raises no asynchronous status, writes Delta, work and info only. SCG_ERR_INVALID, nothing launched, in
 * this sequence: a null ctx, F not a positive multiple of 16 up to SCG_RIDGE_MAX_F, n_mat outside [1, SCG_GRAM_MAX_SEGMENTS], n_rhs
 * outside [1, SCG_GRAM_MAX_TARGETS], a null array. */
#define SCG_RIDGE_MAX_F 4096
int scg_ridge_solve(scg_ctx *ctx, int32_t F, int32_t n_mat, int32_t n_rhs, const float *A, const float *B, const double *lam,
                    const double *mu /* HOST [n_mat] */, const uint8_t *skip /* HOST [n_mat] */, double *work /* [n_mat][F][F] */,
                    double *Delta /* [n_mat][n_rhs][F] */, int32_t *info /* [n_mat] */, void *stream);
/* Option.policy value part (SPEC §3.1): q[5][n] = Q_k(s, .) for one VF Wk[5][1296]. */
int scg_q_values(scg_ctx *ctx, int32_t n, const float *x, const float *y, const float *vx,
                 const float *vy, const float *Wk, float *q, void *stream);
/* ---- lambda-return targets (SPEC §27): one greedy value per recorded row, and the backward scan over every env's rows.
 * Reporting instruments of the value fits: nothing acts or learns with them. Both need no map and raise no asynchronous status. */
#define SCG_ROW_NONE 255   /* a row's table entry that names no table */
/* Row values (SPEC §27.1): v[i] = max_a Q_{tab[i]}(s_i, a) for the table W[tab[i]][5][1296], and a[i] the lowest index that attains it.
 * Each Q has the bits scg_q_values gives for Wk = W[tab[i]] (SPEC §3.1's order); the max is SPEC §5's (m = Q[0]; m = max(m, Q[1]);
 * ...). A row with tab[i] == SCG_ROW_NONE or tab[i] >= n_tab gets v = +0, a = 255, and its state is not read. n_tab in [1, n_vf]. The
 * same bits from every block build and every launch geometry. Preconditions and stream behaviour are scg_q_values'; writes v and a
 * only; n = 0 succeeds and writes nothing. SCG_ERR_INVALID, nothing launched, in this sequence: a null ctx, n < 0, a null array other
 * than a, n_tab out of range. */
int scg_row_values(scg_ctx *ctx, int64_t n, const float *x, const float *y, const float *vx, const float *vy,
                   const uint8_t *tab, const float *W /* [n_tab][5][1296] */, int32_t n_tab,
                   float *v /* [n] */, uint8_t *a /* [n], may be NULL */, void *stream);
/* Lambda returns (SPEC §27.2) of a record in (env, row) order: env e owns rows offsets[e] .. offsets[e + 1] - 1 of the `total` rows (the
 * kernel clamps both ends into [0, total], so no offsets make it read or write outside the arrays). Per env, in binary64, every
 * operation rounded once and none fused, backwards from the env's last row: the root stream y0 on every row (r; r + gamma v0 on the
 * last row of a record cut before its episode ended; else r + gamma ((1 - lam) v0 + lam y0')) and the option stream yk on the rows with
 * vf >= 1 (+0 elsewhere), which carries r_option_success on a SUCCESS row, goes over to the root stream where the option ends (term
 * != 0) and bootstraps from vk while it goes on. Row 0 of an env is its begin row: +0 both. SPEC §27.2 has every case. A non-finite
 * value leaves its env's outputs unspecified from that row backwards. Writes y0 and yk only. SCG_ERR_INVALID, nothing launched: a
 * null ctx, n_env < 0, total < 0, a null array, gamma or lam outside [0, 1] or NaN. */
int scg_lambda_returns(scg_ctx *ctx, int32_t n_env, const int64_t *offsets /* DEVICE [n_env + 1] */, int64_t total,
                       const float *reward, const uint8_t *done, const uint8_t *vf, const uint8_t *term,
                       const float *v0, const float *vk, double gamma, double lam, double r_option_success,
                       double *y0, double *yk /* [total] */, void *stream);
/* Trace returns (SPEC §28.1): scg_lambda_returns' scan with a trace coefficient per row. action[i] is row i's recorded action, ag[i] the
 * greedy action at row i's state of the table that acts on row i + 1 (255: none). A row i that is not its env's row 0 carries
 *   c_i = ((flags & SCG_TRACE_CUT) && action[i] != ag[i - 1]) ? +0 : lam_vf[vf[i] < n_lam ? vf[i] : 0]
 * (selected, never computed), and the mix at local row j is (1 - c) b + c y' with c = c_{j+1}, 1 - c formed per row by one binary64
 * subtraction; every case of the two streams is scg_lambda_returns'. Rows without a row j + 1 in their env read no coefficient.
 * h (optional) is the root stream's effective length: +0 on row 0, 1 on a done row and on an env's last row, else 1 + c_{j+1} h_{j+1};
 * with h == NULL nothing of it is formed. lam_vf is a HOST array of n_lam values, n_lam in [1, n_vf]. Without SCG_TRACE_CUT and with
 * every lam_vf[k] = lam, y0 and yk are scg_lambda_returns' at lam by bits; so they are with the flag where action[i] == ag[i - 1] on
 * every row whose coefficient is read; with the flag and no such row they are scg_lambda_returns' at lam = 0. Writes y0, yk and h only.
 * SCG_ERR_INVALID, nothing launched, in this sequence: a null ctx, n_env < 0, total < 0, a null array other than h, n_lam out of
 * range, gamma or a lam_vf[k] outside [0, 1] or NaN, flag bits other than SCG_TRACE_CUT. n_env = 0 and total = 0 succeed and write
 * nothing. */
#define SCG_TRACE_CUT 1u   /* cut the trace where the recorded action is not the greedy one (Watkins) */
int scg_trace_returns(scg_ctx *ctx, int32_t n_env, const int64_t *offsets /* DEVICE [n_env + 1] */, int64_t total,
                      const float *reward, const uint8_t *done, const uint8_t *vf, const uint8_t *term,
                      const uint8_t *action, const uint8_t *ag /* [total] */,
                      const float *v0, const float *vk,
                      double gamma, const double *lam_vf /* HOST [n_lam] */, int32_t n_lam, uint32_t flags,
                      double r_option_success,
                      double *y0, double *yk, double *h /* [total]; h may be NULL */, void *stream);
/* Cross row values (SPEC §29.1): the value under one table of the action another table selects. For a row with a table k = tab[i] <
 * n_tab: qs = Q^sel_k(s_i, .) and qv = Q^val_k(s_i, .) under W_sel[k] and W_val[k], each with the bits scg_q_values gives for that Wk;
 * m = SPEC §5's max of qs, a* the lowest index that attains it (scg_row_values' rule: five NaNs give index 0); vs[i] = m, a[i] = a*,
 * v[i] = qv[a*], selected by a chain of constant-index compares and never recomputed. With SCG_CROSS_GIVEN a* = act[i], only W_val is
 * contracted (W_sel is not read and may be NULL), vs must be NULL, and a row with act[i] >= 5 is a row without a table. A row without
 * a table (tab[i] == SCG_ROW_NONE or tab[i] >= n_tab) gets v = +0, a = 255, vs = +0, and its state is not read. With W_val == W_sel, v
 * and a are scg_row_values' by bits and vs == v. The same bits from every block build and every launch geometry. Preconditions, stream
 * behaviour and n = 0 are scg_row_values'; writes v, a and vs only. SCG_ERR_INVALID, nothing launched, in this sequence: a null ctx,
 * n < 0, a null array other than a, vs, act (flag clear) and W_sel (flag set), n_tab outside [1, n_vf], flag bits other than
 * SCG_CROSS_GIVEN, act == NULL or vs != NULL with the flag. */
#define SCG_CROSS_GIVEN 1u   /* the selecting action is act[i]; W_sel is not read */
int scg_row_values_cross(scg_ctx *ctx, int64_t n, const float *x, const float *y, const float *vx, const float *vy,
                         const uint8_t *tab, const float *W_sel, const float *W_val /* [n_tab][5][1296] each */, int32_t n_tab,
                         const uint8_t *act /* [n]; with SCG_CROSS_GIVEN only, else NULL */, uint32_t flags,
                         float *v /* [n] */, uint8_t *a /* [n], may be NULL */, float *vs /* [n], may be NULL */, void *stream);
/* ---- the device record store (SPEC §30.1): a record from the launch buffers to the operands of a value fit without leaving the device.
 * A store keeps, for n envs with room for cap rows each, one [n][cap] array per field of scg_record (element (e, r) at e * cap + r; any
 * may be NULL = not kept), have[n] (rows held per env) and overflow[1] (rows dropped so far); the caller zeroes have and overflow once.
 * HOST struct of DEVICE pointers. All three calls are stream-ordered, sync nothing, need no map, raise no asynchronous status and give
 * the same bits from every block build. */
typedef struct {
    float *x, *y, *vx, *vy, *reward;       /* [n][cap]; any may be NULL = not kept */
    uint8_t *action, *done, *vf, *term;
    int8_t *option_id;
    int32_t *have;                         /* [n], required */
    int32_t *overflow;                     /* [1], required */
} scg_record_store;
/* Append one launch's rows: for every env e of launch->n, dst[e * cap + have[e] + r] = src[r * n + e] for r < len[e] in every field kept
 * on both sides (a field NULL on either side is skipped), then have[e] += len[e]. Rows that would pass cap are dropped: have[e] stops
 * at cap and overflow[0] grows by their number. len is read clamped into [0, rows], have into [0, cap]; nothing else is written.
 * launch->first is not read: the store's env e is the launch's column e. SCG_ERR_INVALID, nothing launched, in this sequence: a null
 * ctx, a null launch or store, launch->len, store->have or store->overflow NULL, launch->n < 1, launch->rows < 1, cap < 1. */
int scg_record_append(scg_ctx *ctx, const scg_record *launch, const scg_record_store *store, int32_t cap, void *stream);
/* offsets[e] = have[0] + ... + have[e - 1], offsets[n] the total: the exclusive scan, int64. n = 0 writes offsets[0] = 0.
 * SCG_ERR_INVALID, nothing launched: a null ctx, n < 0, offsets NULL, have NULL with n > 0. */
int scg_record_offsets(scg_ctx *ctx, int32_t n, const int32_t *have, int64_t *offsets /* DEVICE [n + 1] */, void *stream);
/* Pack the store into the flat record in (env, row) order: flat row offsets[e] + r holds env e's row r, field by field (a flat array
 * that is NULL is skipped). Optional outputs, each [total], skipped when NULL: env[i] and row[i] (the flat row's env and local row) and
 *   tab0[i] = done == 0 ? 0 : SCG_ROW_NONE
 *   tabk[i] = (vf >= 1 && term == 0 && done == 0) ? vf : SCG_ROW_NONE
 *   tabA[i] = (row i + 1 is the same env's && (row == 0 || done == 0)) ? vf[i + 1] : SCG_ROW_NONE
 * the row tables of the lambda-return targets (a begin row carries done = 2 and ends no episode). The kernel clamps every env's range
 * into [0, total] as the scans do and cuts it to cap rows: no offsets make it read outside the store or write outside [0, total).
 * Writes the flat arrays given and nothing else. SCG_ERR_INVALID, nothing launched, in this sequence: a null ctx, n < 0, cap < 1,
 * total < 0, a null store or offsets, a flat array whose field the store does not keep, a table without the store's done, vf and
 * term. n = 0 and total = 0 succeed and write nothing. */
int scg_record_pack(scg_ctx *ctx, int32_t n, int32_t cap, const scg_record_store *store, const int64_t *offsets /* DEVICE [n + 1] */,
                    int64_t total, float *x, float *y, float *vx, float *vy, float *reward, uint8_t *action, uint8_t *done,
                    uint8_t *vf, uint8_t *term, int8_t *option_id /* flat [total]; any may be NULL */,
                    int32_t *env, int32_t *row, uint8_t *tab0, uint8_t *tabk, uint8_t *tabA /* [total]; any may be NULL */,
                    void *stream);
/* SkillChainingAgent.q_update on explicit transitions for one VF (SPEC §5): accumulates G_k and n_k
 * into the ctx gradient buffers at VF index k (other VFs zeroed), optionally applies to Wk_all. */
int scg_q_update(scg_ctx *ctx, int32_t n, int32_t k, const float *x, const float *y, const float *vx,
                 const float *vy, const uint8_t *action, const float *r, const float *cont,
                 const float *xn, const float *yn, const float *vxn, const float *vyn, float *W,
                 uint32_t flags, void *stream);
/* Option.initiation_classifier.predict (SPEC §4.1): out[n] u8 = w.psi(x,y) > 0 for one row w8[8]. */
int scg_classifier_predict(scg_ctx *ctx, int32_t n, const float *x, const float *y, const float *w8,
                           uint8_t *out, void *stream);
/* The value whose sign scg_classifier_predict tests (SPEC §24.2): z[n] f32 = w.psi(x,y) by the same device function, so
 * (z > 0) == out for every input, NaN included. scg_classifier_predict's checks in its sequence; n = 0 writes nothing;
 * needs no map; writes z only. */
int scg_classifier_logits(scg_ctx *ctx, int32_t n, const float *x, const float *y, const float *w8,
                          float *z, void *stream);
/* Option.initiation_classifier.fit (SPEC §6), batched over n_fit options: xy[M_total][2],
 * label[M_total] u8, offsets[n_fit+1] int32 (device), w[n_fit][8] in/out. */
int scg_fit_initiation(scg_ctx *ctx, int32_t n_fit, const float *xy, const uint8_t *label,
                       const int32_t *offsets, float *w, int32_t iters, float lr, float l2, void *stream);

/* Option graph (SPEC §4.2): parents[k] for k = 1..n_options (HOST int32[n_options+1], entry 0
 * ignored) = the option whose initiation set option k targets, 0 = the task goal. Default: the chain
 * k -> k-1. Must be acyclic (every option reaches the goal). */
int scg_set_option_parents(scg_ctx *ctx, const int32_t *parents);

/* A learning scg_step also prepares the env order (SPEC §5) of the next step from the option ids it leaves.
 * Call this after writing `option_id` by any other means (a reset, a restored checkpoint): the next scg_step
 * then sorts afresh. Without it the step is still correct for the ids it finds, but groups and sums them in
 * the stale order (slower, and not the canonical rounding). A different `option_id` pointer is noticed
 * automatically. */
int scg_invalidate_order(scg_ctx *ctx);

/* ---- outer-loop support (SPEC §7): device-resident trajectory ring + per-step events,
 * so that the host skill-discovery loop never has to read env state every step.
 * scg_set_trace_buffers: caller-owned device buffers filled by every following scg_step (NULLs disable):
 *   ring_x, ring_y  f32[ring_len][N]  position of s_t at row (ep_steps at entry) & (ring_len-1); ring_len = 2^m
 *   events          u8[N]   bit 0 = reached the goal this step; bit k (1..5) = s' lies in initiation set k
 *   ev_len          i32[N]  states recorded so far in the env's episode (ep_steps at entry + 1)
 * scg_harvest: for each listed env (device int32 list, caller-sorted) emit L_pos + L_neg examples taken
 * backwards from the most recent recorded state: out_xy[n_sel][L][2], out_label[n_sel][L] u8 with
 * 1 = one of the last L_pos states, 0 = older, 255 = no such state (episode too short / ring overwritten). */
int scg_set_trace_buffers(scg_ctx *ctx, float *ring_x, float *ring_y, int32_t ring_len, uint8_t *events,
                          int32_t *ev_len);
int scg_harvest(scg_ctx *ctx, int32_t n_sel, const int32_t *sel_env, const float *ring_x, const float *ring_y,
                int32_t ring_len, const int32_t *ev_len, int32_t l_pos, int32_t l_neg, float *out_xy,
                uint8_t *out_label, void *stream);

/* scg_collect_examples: the device-side creation trigger (SPEC §7), one launch, nothing returns to the host: every env
 * whose `events` byte has one of `event_bits` set — with prev_in (u8[N], in/out) only on the step the bit goes up —
 * appends its min(L, ev_len, ring_len) most recent ring states behind the *count (device int32, in/out) examples
 * already in ex_xy[cap][2] / ex_label[cap] (1 = one of the last l_pos states, 0 = older), in env order; what does not
 * fit is dropped. The trace buffers of scg_set_trace_buffers are read. *count = min(cap, *count + rows); cap = 0 is admitted
 * (nothing is written, *count becomes 0). A negative *count is not an error: rows whose position falls outside [0, cap) are
 * dropped, so nothing is ever written in front of the buffer, and *count = min(cap, *count + rows) as usual (the same holds
 * for scg_collect_frontier's count[p]). Refused (SCG_ERR_INVALID, nothing launched): event_bits = 0, l_pos or l_neg < 0,
 * l_pos + l_neg < 1 or beyond INT32_MAX (the sum is formed in 64 bits by all four collector entry points), cap < 0, a null
 * ex_xy / ex_label / count. */
int scg_collect_examples(scg_ctx *ctx, uint32_t event_bits, uint8_t *prev_in, int32_t l_pos, int32_t l_neg,
                         float *ex_xy, uint8_t *ex_label, int32_t *count, int32_t cap, void *stream);
/* Optional: announce the trigger the NEXT scg_collect_examples will be called with (same event_bits, prev_in, l_pos + l_neg and
 * count). Every following scg_step then leaves the per-row example totals behind while it commits its results (the rows are
 * the same), and a matching scg_collect_examples right after it needs one launch instead of two. Results are identical either
 * way; a call that does not match the announcement, or comes without a step in between, takes the two-launch path.
 * event_bits = 0 withdraws the announcement. prev_in and count are READ by every following scg_step until then (device
 * pointers kept in the ctx): keep them alive, or withdraw the announcement before freeing them. scg_step checks them best-effort
 * (hipPointerGetAttributes: memory handed back to the DRIVER is noticed and refused with SCG_ERR_STATE; memory a caching allocator
 * such as torch's has merely recycled still reads as a device allocation and is NOT noticed) — the rule above is the contract.
 * The step also takes its copy of *count (the level the one-launch collect appends behind) while it commits. So between a
 * scg_step and the matching scg_collect_examples behind it the caller must not write *count or prev_in: a fill level reset
 * there would be ignored and the rows appended behind the old one. Reset them after the collect (before the next scg_step),
 * or withdraw the announcement first; scg_collect_examples itself and scg_arm_collect both drop the step's totals, so a
 * second collect without a step in between reads the buffers afresh. (SkillChainingAgent resets a level only when an
 * option's collection starts or ends, never between a step-batch and its collect.) */
int scg_arm_collect(scg_ctx *ctx, uint32_t event_bits, const uint8_t *prev_in, int32_t l_pos, int32_t l_neg, const int32_t *count);
/* scg_collect_frontier: frontier collection for skill-tree growth (SPEC §13), two launches, nothing returns to the host. Nodes
 * p = 0..n_options: node 0 is the goal (events bit 0), node p >= 1 initiation set p (events bit p). An env with ev_len >= 1
 * hits node p when bit p of target_mask and of its events byte are set and its s_t = ring[(ev_len-1) & (ring_len-1)] lies in
 * no initiation set of cover_mask (SPEC §4.1's z > 0 with clf row k, f32[n_vf][8]; no `known` term); it then appends its
 * min(l_pos + l_neg, ev_len, ring_len) most recent ring states behind count[p] in node p's buffer ex_xy[n_vf][cap][2] /
 * ex_label[n_vf][cap] (1 = one of the last l_pos states, 0 = older), in env order; what does not fit is dropped and
 * count[p] = min(cap, count[p] + rows). An env may hit several nodes. Stateless: no prev_in, and an announced
 * scg_arm_collect trigger is neither read nor cleared. Refused (SCG_ERR_INVALID, nothing launched): target_mask bits at or
 * beyond n_vf, cover_mask bit 0 or bits beyond n_options, a target option outside cover_mask, cap < 1, l_pos or l_neg < 0,
 * l_pos + l_neg < 1, a null pointer; SCG_ERR_STATE without trace buffers. target_mask = 0 appends nothing. */
int scg_collect_frontier(scg_ctx *ctx, uint32_t target_mask, uint32_t cover_mask, const float *clf, int32_t l_pos, int32_t l_neg,
                         float *ex_xy, uint8_t *ex_label, int32_t *count, int32_t cap, void *stream);

/* Gestation (SPEC §4.4; Konidaris & Barto 2009: a new option learns off-policy before it may run). Bit k of gest_mask:
 * option k's classifier is in use (initiation / target tests, event bits) but the option is never selected; every env
 * whose state lies in its initiation set contributes an off-policy TD item to VF k; succ_counts[k] (device int32[n_vf],
 * caller-owned, may be NULL) counts the transitions that reached option k's target from inside its initiation set.
 * The caller moves the bit from gest_mask to scg_step's enabled_mask when the count is high enough. */
int scg_set_gestation(scg_ctx *ctx, uint32_t gest_mask, int32_t *succ_counts);

/* ---- asynchronous failures ----
 * Launches are asynchronous, so a kernel that has to give up cannot return a status. It leaves its outputs untouched
 * and ORs a reason into a host-visible status word owned by the ctx; from then on EVERY entry point that would launch
 * work returns SCG_ERR_ASYNC (scg_last_error names the reason) until scg_clear_async_error is called. Today one
 * kernel can do this: scg_fit_initiation's — the eight workgroups of a fit problem exchange partial sums through
 * memory every iteration and need to be running at the same time; if the card is shared (another stream, another
 * process) a workgroup may be kept off it. A missing partner is waited for scg_set_fit_timeout seconds of wall clock
 * (default 2 s), then the fit of that problem is abandoned: its row of `w` keeps the values it had, never a partial
 * result or a NaN. Word layout: SCG_ASYNC_FIT_TIMEOUT | 0x100 << (problem index & 15).
 * The step kernel is the second: the wavefront subsets of a workgroup hand work to each other through counters in LDS and
 * poll them with a bound (2^20 rounds; every awaited count is produced by wavefronts that never wait on the waiter, so
 * the bound is only reached through a logic error or a hung wavefront). A poll that runs out raises
 * SCG_ASYNC_STEP_HANDOFF: that block's partial gradients are dropped (its slab counts read 0) and the step's other
 * outputs for the block's envs are unspecified — the state must be restored from a checkpoint.
 * The peer exchange is the third (scg_peer_exchange_apply): SCG_ASYNC_PEER_TIMEOUT when a peer's epoch does not arrive in
 * time, SCG_ASYNC_STEP_HANDOFF on every rank when any rank's step of that exchange was void; W is untouched in both cases.
 *   scg_async_status      the word (optional out) and its status; `synchronize` != 0 waits for `stream` first, which
 *                         makes the answer final for everything launched on it so far
 *   scg_decode_async_word the same mapping word -> status + text without a ctx (pure host code) */
#define SCG_ASYNC_FIT_TIMEOUT 0x1u
#define SCG_ASYNC_STEP_HANDOFF 0x2u
#define SCG_ASYNC_PEER_TIMEOUT 0x4u   /* scg_peer_exchange_apply: a peer's epoch did not arrive within scg_set_peer_timeout; W untouched */
int scg_async_status(scg_ctx *ctx, void *stream, int32_t synchronize, uint32_t *word_out);
int scg_clear_async_error(scg_ctx *ctx);
int scg_set_fit_timeout(scg_ctx *ctx, double seconds);
int scg_set_peer_timeout(scg_ctx *ctx, double seconds);     /* the peer wait's bound (default 2 s), see scg_peer_exchange_apply */
int scg_decode_async_word(uint32_t word, char *buf, int32_t buf_len);
/* test hook: raise bits of the status word from the host, as a kernel would */
int scg_debug_raise_async(scg_ctx *ctx, uint32_t word);

/* ---- measurement hooks (bench.py's roofline leg) ----
 * scg_profile_reset(ctx, p) with p >= 1 makes every p-th following scg_step record a HIP event pair round
 * its fused kernel on the launch stream (each pair costs a few microseconds of queue bubble, so sampling
 * perturbs the timed region less); scg_profile_read synchronises those events and returns the summed
 * kernel time (ms) and the number of launches measured; scg_profile_reset(ctx, 0) stops recording. */
int scg_profile_reset(scg_ctx *ctx, int32_t enable);
int scg_profile_read(scg_ctx *ctx, double *kernel_ms_sum, int64_t *launches);

#ifdef __cplusplus
}
#endif
#endif
