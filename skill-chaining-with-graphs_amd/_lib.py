"""ctypes binding of libscg_hip.so (include/scg_abi.h). The product path has NO fallback: if the HIP
library is missing or a call fails, this module raises — it never routes to a CPU implementation."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SCG_LIB") or os.path.join(_HERE, "csrc", "libscg_hip.so")   # SCG_LIB: A/B builds

NUM_ACTIONS = 5
FOURIER_ORDER = 5
NUM_FEATURES = 1296
W_ROW = NUM_ACTIONS * NUM_FEATURES     # one value function's weights: W is [n_vf] of these, a packed operand [n_vf] of W_ROW + 1
MAX_OPTIONS = 5
MAX_EDGES = 256
CLF_STRIDE = 8

STEP_LEARN = 1
STEP_APPLY = 2
STEP_INTERRUPT = 4   # include/scg_abi.h SCG_STEP_INTERRUPT: SPEC §12, the interrupting learner (with STEP_LEARN only)
ROLLOUT_BEGIN = 1          # include/scg_abi.h SCG_ROLLOUT_*
ROLLOUT_ONE_EPISODE = 2
ROLLOUT_BEGIN_AT = 4
ROLLOUT_MAX_STEPS = 1024
TRIAL_SUCCESS = 1          # include/scg_abi.h SCG_TRIAL_*: the outcome of an option trial (0: not run)
TRIAL_EPISODE_END = 2
TRIAL_LEFT_INITIATION = 3
TRIAL_TIMEOUT = 4
TRIAL_MAX_STEPS = ROLLOUT_MAX_STEPS
ROLLOUT_TERM_INTERRUPTED = 5   # include/scg_abi.h SCG_ROLLOUT_TERM_INTERRUPTED: a recorded row's term where an option was interrupted
SELECT_INTERRUPT = 1       # include/scg_abi.h SCG_SELECT_*: the rules of scg_rollout_select (SPEC §11, §14)
SELECT_BEST = 2
POP_MAX = 64               # SCG_POP_MAX: the policies of one population rollout (SPEC §21)
NO_FIRST_ACTION = 255      # SPEC §19: scg_rollout_branch's first_action entry of an env that is not forced (any value >= NUM_ACTIONS)
BRANCH_ID_BASE = 2 ** 40   # the global env ids of branch rollouts start here: no stream of a record (env_id_base = 0) is reused
ABI_VERSION = 5            # include/scg_abi.h SCG_ABI_VERSION
ASYNC_FIT_TIMEOUT = 0x1
ASYNC_STEP_HANDOFF = 0x2
ASYNC_PEER_TIMEOUT = 0x4
PEER_HANDLE_BYTES = 64      # hipIpcMemHandle_t
PEER_MAX_RANKS = 8
GRAM_SLAB = 1024            # include/scg_abi.h SCG_GRAM_*: SPEC §16.1's slab, the segment cap, one workgroup's block of A (features a side)
GRAM_MAX_SEGMENTS = 64
GRAM_MACRO_TILE = 96
GRAM_MAX_TARGETS = 16       # include/scg_abi.h SCG_GRAM_MAX_TARGETS: SPEC §20.1's right-hand sides per call (the columns of one MFMA operand)
CROSS_GRAM_MACRO_TILE = 96  # include/scg_abi.h SCG_CROSS_GRAM_MACRO_TILE: one workgroup's block of SPEC §17.1's C (rows and columns alike)
BASIS_ORDERS = (3, 5, 7)    # SPEC §18: the orders of the basis-order probe (F = (order + 1)^4 = 256, 1296, 4096 features)
BASIS_VALUES_MAX_ROWS = 8   # include/scg_abi.h SCG_BASIS_VALUES_MAX_ROWS
ROW_NONE = 255              # include/scg_abi.h SCG_ROW_NONE: SPEC §27.1's table entry of a row without a table
TRACE_CUT = 1               # include/scg_abi.h SCG_TRACE_CUT: SPEC §28.1's flag of scg_trace_returns
CROSS_GIVEN = 1             # include/scg_abi.h SCG_CROSS_GIVEN: SPEC §29.1's flag of scg_row_values_cross
RIDGE_TILE = 16             # SPEC §31: the matrix side of scg_ridge_solve is a positive multiple of it ...
RIDGE_MAX_F = 4096          # ... up to include/scg_abi.h SCG_RIDGE_MAX_F


def basis_features(order: int) -> int:
    """F of SPEC §18's basis of order `order`."""
    if order not in BASIS_ORDERS:
        raise ScgError(f"the basis order must be one of {BASIS_ORDERS}")
    return (int(order) + 1) ** 4


class ScgError(RuntimeError):
    pass


class ScgConfig(C.Structure):
    _fields_ = [
        ("n_envs", C.c_int32),
        ("n_options", C.c_int32),
        ("fourier_order", C.c_int32),
        ("device", C.c_int32),
        ("env_id_base", C.c_int64),
        ("seed", C.c_uint64),
        ("gamma", C.c_float),
        ("alpha", C.c_float),
        ("epsilon", C.c_float),
        ("r_option_success", C.c_float),
        ("max_episode_steps", C.c_int32),
        ("max_option_steps", C.c_int32),
        ("update_count_floor", C.c_int32),
        ("reoffer_period", C.c_int32),
    ]


class RolloutStats(C.Structure):
    """scg_rollout_stats: device pointers of the per-env counters of SPEC §8 (NULL = not kept)."""
    _fields_ = [
        ("ep_return", C.c_void_p),
        ("ret_sum", C.c_void_p),
        ("episodes", C.c_void_p),
        ("goals", C.c_void_p),
        ("len_sum", C.c_void_p),
        ("vf_steps", C.c_void_p),
        ("entries", C.c_void_p),
        ("declines", C.c_void_p),
        ("successes", C.c_void_p),
        ("finished", C.c_void_p),
    ]


class TrialOut(C.Structure):
    """scg_trial_out: device pointers of the per-entry outputs of SPEC §9 (outcome required, any other NULL = not written)."""
    _fields_ = [
        ("outcome", C.c_void_p),
        ("steps", C.c_void_p),
        ("ret", C.c_void_p),
        ("disc_ret", C.c_void_p),
        ("v0", C.c_void_p),
        ("end_x", C.c_void_p),
        ("end_y", C.c_void_p),
        ("end_vx", C.c_void_p),
        ("end_vy", C.c_void_p),
    ]


class Record(C.Structure):
    """scg_record: the per-step rows of SPEC §10 for envs / entries first .. first+n-1, rows rows each; device pointers of
    [rows][n] arrays (len [n] required, any other NULL = not recorded)."""
    _fields_ = [
        ("first", C.c_int32),
        ("n", C.c_int32),
        ("rows", C.c_int32),
        ("len", C.c_void_p),
        ("x", C.c_void_p),
        ("y", C.c_void_p),
        ("vx", C.c_void_p),
        ("vy", C.c_void_p),
        ("reward", C.c_void_p),
        ("action", C.c_void_p),
        ("done", C.c_void_p),
        ("vf", C.c_void_p),
        ("term", C.c_void_p),
        ("option_id", C.c_void_p),
    ]


class RecordStore(C.Structure):
    """scg_record_store: SPEC §30.1's device store for n envs of cap rows each; device pointers of one [n][cap] array per record
    field (NULL = not kept), have [n] and overflow [1] (int32, both required)."""
    _fields_ = [
        ("x", C.c_void_p),
        ("y", C.c_void_p),
        ("vx", C.c_void_p),
        ("vy", C.c_void_p),
        ("reward", C.c_void_p),
        ("action", C.c_void_p),
        ("done", C.c_void_p),
        ("vf", C.c_void_p),
        ("term", C.c_void_p),
        ("option_id", C.c_void_p),
        ("have", C.c_void_p),
        ("overflow", C.c_void_p),
    ]


class Audit(C.Structure):
    """scg_audit: device pointers of SPEC §15's per-env audit arrays, each [N] (any NULL = not given / not written)."""
    _fields_ = [
        ("force", C.c_void_p),
        ("applied", C.c_void_p),
        ("cand", C.c_void_p),
        ("v_root", C.c_void_p),
        ("v_cand", C.c_void_p),
        ("disc_ret", C.c_void_p),
        ("disc_g", C.c_void_p),
        ("disc_final", C.c_void_p),
    ]


class Population(C.Structure):
    """scg_population: SPEC §21's C policies over n_per envs each; device pointers of the [C] epsilon (float32) and enabled mask
    (uint32) arrays (NULL = the context's epsilon / the call's enabled_mask for every policy)."""
    _fields_ = [
        ("n_policies", C.c_int32),
        ("n_per", C.c_int32),
        ("epsilon", C.c_void_p),
        ("enabled", C.c_void_p),
    ]


_P = C.c_void_p
# the arguments the rollout and the trial entry points start with; each appends its own tail (record, interrupt counts, stream)
_ROLLOUT = [_P] + [_P] * 13 + [C.c_uint32, C.c_uint64, C.c_int32, C.c_uint32, C.POINTER(RolloutStats)]
_TRIALS = [_P, C.c_int32] + [_P] * 7 + [C.c_uint32, C.c_uint64, C.POINTER(TrialOut)]
_SIGS = {
    "scg_abi_version": (C.c_int, []),
    "scg_block_envs": (C.c_int, []),
    "scg_strerror": (C.c_char_p, [C.c_int]),
    "scg_last_error": (C.c_char_p, [_P]),
    "scg_create": (C.c_int, [C.POINTER(_P), C.POINTER(ScgConfig)]),
    "scg_destroy": (C.c_int, [_P]),
    "scg_set_hparams": (C.c_int, [_P, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "scg_set_map": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P, _P]),
    "scg_step": (C.c_int, [_P] + [_P] * 13 + [C.c_uint32, C.c_uint64, C.c_uint32, _P]),
    "scg_step_gated": (C.c_int, [_P] + [_P] * 13 + [C.c_uint32, C.c_uint64, C.c_uint32, _P, _P, C.c_uint32]),
    "scg_rollout": (C.c_int, _ROLLOUT + [_P]),
    "scg_option_trials": (C.c_int, _TRIALS + [_P]),
    "scg_rollout_record": (C.c_int, _ROLLOUT + [C.POINTER(Record), _P]),
    "scg_option_trials_record": (C.c_int, _TRIALS + [C.POINTER(Record), _P]),
    "scg_rollout_interrupt": (C.c_int, _ROLLOUT + [_P, C.POINTER(Record), _P]),
    "scg_rollout_select": (C.c_int, _ROLLOUT + [_P, _P, C.POINTER(Record), C.c_uint32, _P]),
    "scg_rollout_audit": (C.c_int, _ROLLOUT + [_P, _P, C.POINTER(Record), C.c_uint32, C.POINTER(Audit), _P]),
    "scg_rollout_branch": (C.c_int, _ROLLOUT + [_P, _P, C.POINTER(Record), C.c_uint32, C.POINTER(Audit), _P, _P]),
    "scg_rollout_population": (C.c_int, _ROLLOUT + [_P, _P, C.POINTER(Record), C.c_uint32, C.POINTER(Audit), _P, _P,
                                            C.POINTER(Population)]),
    "scg_rollout_population_clf": (C.c_int, _ROLLOUT + [_P, _P, C.POINTER(Record), C.c_uint32, C.POINTER(Audit), _P, _P,
                                                C.POINTER(Population), _P]),
    "scg_rollout_population_gate": (C.c_int, _ROLLOUT + [_P, _P, C.POINTER(Record), C.c_uint32, C.POINTER(Audit), _P, _P,
                                                 C.POINTER(Population), _P, _P]),
    "scg_grad_buffers": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P)]),
    "scg_set_grad_buffers": (C.c_int, [_P, _P, _P]),
    "scg_apply_update": (C.c_int, [_P, _P, _P, _P, _P]),
    "scg_set_grad_buffer_packed": (C.c_int, [_P, _P]),
    "scg_apply_update_packed": (C.c_int, [_P, _P, _P, _P]),
    "scg_apply_update_slots": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int64, _P]),
    "scg_pinball_step": (C.c_int, [_P, C.c_int32] + [_P] * 7 + [_P]),
    "scg_fourier_features": (C.c_int, [_P, C.c_int32] + [_P] * 5 + [_P]),
    "scg_feature_gram": (C.c_int, [_P, C.c_int64] + [_P] * 5 + [C.c_int32, _P, _P, _P, _P]),
    "scg_feature_gram_targets": (C.c_int, [_P, C.c_int64] + [_P] * 5 + [C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "scg_feature_gram_weighted": (C.c_int, [_P, C.c_int64] + [_P] * 6 + [C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "scg_feature_cross_gram": (C.c_int, [_P, C.c_int64] + [_P] * 8 + [C.c_int32, _P, _P, _P]),
    "scg_basis_features": (C.c_int, [_P, C.c_int32, C.c_int64] + [_P] * 5 + [_P]),
    "scg_basis_gram": (C.c_int, [_P, C.c_int32, C.c_int64] + [_P] * 5 + [C.c_int32, _P, _P, _P, _P]),
    "scg_basis_values": (C.c_int, [_P, C.c_int32, C.c_int64] + [_P] * 5 + [C.c_int32, _P, _P]),
    "scg_logistic_terms": (C.c_int, [_P, C.c_int64] + [_P] * 5 + [_P]),
    "scg_basis_gram_irls": (C.c_int, [_P, C.c_int32, C.c_int64] + [_P] * 6 + [C.c_int32, _P, _P, _P, _P]),
    "scg_row_values": (C.c_int, [_P, C.c_int64] + [_P] * 6 + [C.c_int32, _P, _P, _P]),
    "scg_row_values_cross": (C.c_int, [_P, C.c_int64] + [_P] * 7 + [C.c_int32, _P, C.c_uint32, _P, _P, _P, _P]),
    "scg_lambda_returns": (C.c_int, [_P, C.c_int32, _P, C.c_int64] + [_P] * 6 + [C.c_double] * 3 + [_P, _P, _P]),
    "scg_trace_returns": (C.c_int, [_P, C.c_int32, _P, C.c_int64] + [_P] * 8 + [C.c_double, _P, C.c_int32, C.c_uint32, C.c_double]
                          + [_P] * 4),
    "scg_record_append": (C.c_int, [_P, C.POINTER(Record), C.POINTER(RecordStore), C.c_int32, _P]),
    "scg_record_offsets": (C.c_int, [_P, C.c_int32, _P, _P, _P]),
    "scg_record_pack": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(RecordStore), _P, C.c_int64] + [_P] * 10 + [_P] * 5 + [_P]),
    "scg_ridge_solve": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32] + [_P] * 8 + [_P]),
    "scg_q_values": (C.c_int, [_P, C.c_int32] + [_P] * 6 + [_P]),
    "scg_q_update": (C.c_int, [_P, C.c_int32, C.c_int32] + [_P] * 12 + [C.c_uint32, _P]),
    "scg_classifier_predict": (C.c_int, [_P, C.c_int32] + [_P] * 4 + [_P]),
    "scg_classifier_logits": (C.c_int, [_P, C.c_int32] + [_P] * 4 + [_P]),
    "scg_set_option_parents": (C.c_int, [_P, _P]),
    "scg_invalidate_order": (C.c_int, [_P]),
    "scg_set_trace_buffers": (C.c_int, [_P, _P, _P, C.c_int32, _P, _P]),
    "scg_harvest": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.c_int32, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    "scg_collect_examples": (C.c_int, [_P, C.c_uint32, _P, C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, _P]),
    "scg_arm_collect": (C.c_int, [_P, C.c_uint32, _P, C.c_int32, C.c_int32, _P]),
    "scg_collect_frontier": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, _P]),
    "scg_set_gestation": (C.c_int, [_P, C.c_uint32, _P]),
    "scg_profile_reset": (C.c_int, [_P, C.c_int32]),
    "scg_profile_read": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "scg_fit_initiation": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_float, C.c_float, _P]),
    "scg_async_status": (C.c_int, [_P, _P, C.c_int32, C.POINTER(C.c_uint32)]),
    "scg_clear_async_error": (C.c_int, [_P]),
    "scg_set_fit_timeout": (C.c_int, [_P, C.c_double]),
    "scg_set_peer_timeout": (C.c_int, [_P, C.c_double]),
    "scg_peer_export": (C.c_int, [_P, _P]),
    "scg_peer_open": (C.c_int, [_P, C.c_int32, C.c_int32, _P]),
    "scg_peer_exchange_apply": (C.c_int, [_P, _P, _P]),
    "scg_decode_async_word": (C.c_int, [C.c_uint32, C.c_char_p, C.c_int32]),
    "scg_debug_raise_async": (C.c_int, [_P, C.c_uint32]),
}
EXPORTED_SYMBOLS = tuple(_SIGS)

BLOCK_ENVS_DEFAULT = 256
BLOCK_ENVS_BUILDS = (64, 128, 256)     # SPEC §5 geometry is a build parameter: csrc/Makefile builds one library per value

CHIP_CUS = 256            # MI355X: 8 XCDs x 32 CUs; one 16-wavefront workgroup owns a CU


def auto_block_envs(n_envs: int) -> int:
    """The SPEC §5 block size a context of `n_envs` envs picks when none is given: the SMALLEST build whose workgroups — one per
    block, one per CU — still fit the chip in one round (a workgroup is an ~80 us latency chain whatever its size, so below 65 536
    envs smaller blocks on more CUs win; DESIGN §3.6: 4096 envs 127 / 104 / 69 M env-steps/s at 64 / 128 / 256). Deterministic in
    n_envs alone (the CU count is the chip's constant, not queried): a run's geometry is part of its identity like its seed."""
    for b in BLOCK_ENVS_BUILDS:
        if -(-int(n_envs) // b) <= CHIP_CUS:
            return b
    return BLOCK_ENVS_DEFAULT


_libs = {}


def lib_path(block_envs: int | None = None) -> str:
    """The library of a block geometry: libscg_hip.so (256 envs per block = per workgroup, the throughput build) or
    libscg_hip_b64.so / _b128.so (the small-batch builds). SCG_LIB overrides the default build only."""
    if block_envs in (None, BLOCK_ENVS_DEFAULT):
        return LIB_PATH
    if block_envs not in BLOCK_ENVS_BUILDS:
        raise ScgError(f"block_envs must be one of {BLOCK_ENVS_BUILDS}")
    return os.path.join(_HERE, "csrc", f"libscg_hip_b{block_envs}.so")


def load(block_envs: int | None = None, path: str | None = None) -> C.CDLL:
    """Load the HIP library of a block geometry (once each). Raises ScgError loudly when it has not been built.
    `path`: a variant build of the same ABI (timing / fault-injection builds of csrc/Makefile) instead of the geometry's library."""
    key = (BLOCK_ENVS_DEFAULT if block_envs is None else int(block_envs)) if path is None else os.path.abspath(path)
    if key in _libs:
        return _libs[key]
    if path is None:
        path = lib_path(key)
    if not os.path.exists(path):
        raise ScgError(
            f"{path} is missing: the HIP extension has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C "
            f"{os.path.dirname(path)}`). There is no CPU fallback."
        )
    lib = C.CDLL(path)
    try:
        ver = int(lib.scg_abi_version())
    except AttributeError:
        raise ScgError(f"{path} does not export scg_abi_version: not a libscg_hip.so") from None
    if ver != ABI_VERSION:
        raise ScgError(f"{path} implements ABI version {ver}, this binding expects {ABI_VERSION} "
                       "(include/scg_abi.h): rebuild the library (a stale .so?)")
    for name, (res, args) in _SIGS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise ScgError(f"{path} does not export {name} although it reports ABI version {ver}: rebuild it") from None
        fn.restype = res
        fn.argtypes = args
    if block_envs is not None and isinstance(key, int) and int(lib.scg_block_envs()) != key:
        raise ScgError(f"{path} is built for {int(lib.scg_block_envs())}-env blocks, not {key}: rebuild it")
    _libs[key] = lib
    return lib


def block_envs(block_envs: int | None = None) -> int:
    """SPEC §5 block size of a loaded library (envs whose update items share one accumulation chain)."""
    return int(load(block_envs).scg_block_envs())


def check(status: int, ctx, what: str, lib: C.CDLL) -> None:
    """Raise ScgError for a failed call of `lib`. The text comes from that library: a context's own lives in the context, the
    text of a call without one (a refused scg_create) in a thread_local of the build that refused."""
    if status != 0:
        raise ScgError(f"{what or 'scg call'} failed ({lib.scg_strerror(status).decode()}): {lib.scg_last_error(ctx).decode()}")
