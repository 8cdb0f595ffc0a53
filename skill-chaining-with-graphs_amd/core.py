"""ScgContext — thin, checked Python wrapper over the C-ABI (include/scg_abi.h).

PyTorch is plumbing here: it owns device memory and the stream; every computation happens in the HIP
kernels behind libscg_hip.so. Operand shapes/dtypes/devices are validated on the host before any
launch (a kernel fault can take the whole GPU host down)."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import (CLF_STRIDE, MAX_OPTIONS, NUM_ACTIONS, NUM_FEATURES, STEP_APPLY, STEP_INTERRUPT, STEP_LEARN, W_ROW, ScgConfig,
                   ScgError)
from .maps import PinballMap


def fourier_scale_table(order: int = 5, n_vars: int = 4) -> np.ndarray:
    """SPEC §3: scale_f = 1/||c||_2 (1 for c = 0), float64 then rounded; canonical feature order."""
    n = order + 1
    idx = np.arange(n ** n_vars)
    c = np.stack([(idx // n ** (n_vars - 1 - d)) % n for d in range(n_vars)], 1).astype(np.float64)
    norm = np.sqrt((c * c).sum(1))
    norm[0] = 1.0
    return (1.0 / norm).astype(np.float32)


def _ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def _chk_W(ctx, W: torch.Tensor, name: str = "W") -> torch.Tensor:      # (these three take the context: a stand-in's, too)
    return ctx._chk(W, torch.float32, ctx.n_vf * W_ROW, name)


def _chk_clf(ctx, clf: torch.Tensor) -> torch.Tensor:
    return ctx._chk(clf, torch.float32, ctx.n_vf * CLF_STRIDE, "clf")


def _chk_packed(ctx, gp: torch.Tensor, name: str, rows: int = 1) -> torch.Tensor:      # (a packed operand: G, then the counts)
    return ctx._chk(gp, torch.float32, rows * ctx.n_vf * (W_ROW + 1), name)


class ScgContext:
    # r_option_success defaults to 0: with SPEC §4.2's value-gated entry an option is entered where its value function promises at
    # least the root's, and both estimate the TASK's return (an option that ends bootstraps from the root) — a completion bonus
    # inflates the option's side of that comparison (profiles/r05_oracle_chain_curves_*.txt: 10 000 collapses a seed, 0 is best)
    def __init__(self, n_envs: int, n_options: int, pmap: PinballMap, *, device: int = 0, seed: int = 0,
                 env_id_base: int = 0, gamma: float = 0.99, alpha: float = 1e-3, epsilon: float = 0.05,
                 r_option_success: float = 0.0, max_episode_steps: int = 10000,
                 max_option_steps: int = 250, update_count_floor: int = 0, reoffer_period: int = 4,
                 block_envs: Optional[int] = None,
                 library: Optional[str] = None):
        # SPEC §2's run identity: refused here, before any device call (ctypes would mask them into range silently)
        if not (0 <= int(seed) < 2 ** 64):
            raise ScgError("seed must be a 64-bit unsigned integer")
        if not (-2 ** 63 <= int(env_id_base) < 2 ** 63):
            raise ScgError("env_id_base must be a 64-bit signed integer")
        if not torch.cuda.is_available():
            raise ScgError("no GPU visible to torch: the HIP path cannot run and there is no CPU fallback")
        if not (0 <= n_options <= MAX_OPTIONS):
            raise ScgError(f"n_options must be in [0, {MAX_OPTIONS}]")
        if block_envs is None:                               # SPEC §5 geometry: SCG_BLOCK_ENVS pins it, else by the env count
            block_envs = int(os.environ["SCG_BLOCK_ENVS"]) if os.environ.get("SCG_BLOCK_ENVS") else _lib.auto_block_envs(n_envs)
        # one library per geometry (64 / 128 / 256 envs per block = per workgroup); `library`: a variant build of the same ABI
        self.lib = _lib.load(block_envs) if library is None else _lib.load(None, path=library)
        self.block_envs = int(self.lib.scg_block_envs())
        self.n_envs, self.n_options, self.n_vf = int(n_envs), int(n_options), int(n_options) + 1
        self.device = torch.device("cuda", device)
        self.map = pmap
        self.cfg = ScgConfig(n_envs=n_envs, n_options=n_options, fourier_order=_lib.FOURIER_ORDER,
                             device=device, env_id_base=env_id_base, seed=seed, gamma=gamma, alpha=alpha,
                             epsilon=epsilon, r_option_success=r_option_success,
                             max_episode_steps=max_episode_steps, max_option_steps=max_option_steps,
                             update_count_floor=update_count_floor, reoffer_period=reoffer_period)
        # what later calls attach: the trace tensors, the announced trigger's (prev_in, count), the gradient operand in one of its two
        # forms, SPEC §4.4's success counters; then step()'s cached call
        self._trace = self._armed = self._gbuf = self._gpacked = self._gest_succ = None
        self._step_args = self._step_keep = self._step_fn = self._last_state = None
        self.gest_mask = self.peer_ranks = 0
        self._ctx = C.c_void_p()
        _lib.check(self.lib.scg_create(C.byref(self._ctx), C.byref(self.cfg)), None, "scg_create", self.lib)
        self.scale = fourier_scale_table()
        self.parents = np.arange(-1, n_options, dtype=np.int32).clip(0)      # default chain k -> k-1
        self.set_map(pmap)

    # ------------------------------------------------------------------ plumbing
    def _call(self, name: str, *args) -> None:
        _lib.check(getattr(self.lib, name)(self._ctx, *args), self._ctx, name, self.lib)

    def _stream(self) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _chk(self, t: torch.Tensor, dtype: torch.dtype, numel: int, name: str) -> torch.Tensor:
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != self.device \
                or not t.is_contiguous() or t.numel() != numel:
            raise ScgError(f"{name}: expected contiguous {dtype} tensor with {numel} elements on {self.device}, "
                           f"got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))} "
                           f"on {getattr(t, 'device', '?')}")
        return t

    def close(self) -> None:
        self._step_args = self._step_keep = self._armed = None
        if getattr(self, "_ctx", None) and self._ctx.value:
            self.lib.scg_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    _HPARAMS = ("gamma", "alpha", "epsilon", "r_option_success", "max_episode_steps", "max_option_steps",
                "update_count_floor", "reoffer_period")          # what scg_set_hparams takes (the rest is fixed at create)

    def set_hparams(self, **kw) -> None:
        """Change hyper-parameters between steps. A refused call changes nothing: neither the library's settings nor `cfg`."""
        for k in kw:
            if k not in self._HPARAMS:
                raise ScgError(f"unknown hyper-parameter {k}")
        c = ScgConfig.from_buffer_copy(self.cfg)            # the new settings on a copy: `cfg` follows only an accepted call
        for k, v in kw.items():
            setattr(c, k, v)
        self._call("scg_set_hparams", c.gamma, c.alpha, c.epsilon, c.r_option_success,
                   c.max_episode_steps, c.max_option_steps, c.update_count_floor, c.reoffer_period)
        self.cfg = c

    def set_map(self, pmap: PinballMap) -> None:
        """SPEC §1.1: the map (edges, start list, scalars) of every following step, between steps. Env states are the caller's:
        they must be valid for the new map."""
        edges, starts, sc = pmap.edges, np.ascontiguousarray(pmap.starts, np.float32), pmap.scalars
        self._call("scg_set_map", edges.ctypes.data_as(C.c_void_p), len(edges),
                   starts.ctypes.data_as(C.c_void_p), len(starts), sc.ctypes.data_as(C.c_void_p),
                   self.scale.ctypes.data_as(C.c_void_p))
        self.map = pmap

    # ------------------------------------------------------------------ fused step-batch
    def _step_flags(self, learn: bool, apply: bool, interrupt: bool = False) -> int:
        # (interrupt is passed on as given: without learn the library refuses it, SPEC §12)
        return (STEP_LEARN if learn else 0) | (STEP_APPLY if (learn and apply) else 0) | (STEP_INTERRUPT if interrupt else 0)

    def _chk_operands(self, st: "EnvState", W: torch.Tensor, clf: torch.Tensor, n_tables: int = 1) -> None:
        """The env state, weight and classifier tensors step() and rollout() hand to the library (n_tables: SPEC §21's weight
        tables, one per policy)."""
        N = self.n_envs
        f32, i32, u8 = torch.float32, torch.int32, torch.uint8
        self._chk(st.x, f32, N, "x"); self._chk(st.y, f32, N, "y")
        self._chk(st.vx, f32, N, "vx"); self._chk(st.vy, f32, N, "vy")
        self._chk(st.option_id, i32, N, "option_id"); self._chk(st.opt_steps, i32, N, "opt_steps")
        self._chk(st.ep_steps, i32, N, "ep_steps"); self._chk(st.qcache, f32, NUM_ACTIONS * N, "qcache")
        self._chk(st.action, u8, N, "action"); self._chk(st.reward, f32, N, "reward")
        self._chk(st.done, u8, N, "done")
        self._chk(W, f32, n_tables * self.n_vf * W_ROW, "W"); _chk_clf(self, clf)

    def step(self, st: "EnvState", W: torch.Tensor, clf: torch.Tensor, enabled_mask: int, t: int,
             learn: bool = True, apply: bool = True, interrupt: bool = False, gate: torch.Tensor = None, gate_mask: int = 0) -> None:
        """One fused step-batch (SPEC §1.3-§5). `interrupt` (learning steps only; with learn=False it raises ScgError): SPEC §12's
        interrupting learner — an option that would go on stops where the root's value at the next state is higher, and its
        update item bootstraps from the root's value. `gate` / `gate_mask` (SPEC §26.1, scg_step_gated): a gate table
        [n_vf][2][5][1296] (SPEC §25's layout) on the context's device, and the options (bit k, 1 <= k <= n_options) whose entry
        decisions compare under it instead of under this step's W; gate_mask = 0 is the plain step, and `gate` is then not looked at."""
        if not (0 <= t < 2 ** 64):                            # (before the cached fast path: C.c_uint64 would wrap it silently)
            raise ScgError("step: t must be a 64-bit unsigned step counter")
        gate_mask = int(gate_mask)
        name, tail = "scg_step", ()
        if gate_mask:
            if gate_mask < 0 or (gate_mask & 1) or (gate_mask >> self.n_vf):
                raise ScgError(f"step: gate_mask {gate_mask:#x} names the root or an option beyond the context's {self.n_vf - 1}")
            if not isinstance(gate, torch.Tensor) or tuple(gate.shape) != (self.n_vf, 2, NUM_ACTIONS, NUM_FEATURES):
                raise ScgError(f"step: gate must be a tensor [{self.n_vf}, 2, {NUM_ACTIONS}, {NUM_FEATURES}] (SPEC §25's layout)")
            self._chk(gate, torch.float32, self.n_vf * 2 * W_ROW, "gate")
            name, tail = "scg_step_gated", (_ptr(gate), C.c_uint32(gate_mask))
        # the validated, pre-marshalled pointer arguments of the last call are reused while the same tensors come back
        # (one step is two kernel launches: the host side of a call matters in short runs)
        # (the key holds every tensor's storage address, not only the Python ids: `.data =` / `set_()` on the same object
        # swaps the storage under an unchanged id)
        key = (id(st), id(W), id(clf), st.x.data_ptr(), st.y.data_ptr(), st.vx.data_ptr(), st.vy.data_ptr(),
               st.option_id.data_ptr(), st.opt_steps.data_ptr(), st.ep_steps.data_ptr(), st.qcache.data_ptr(),
               st.action.data_ptr(), st.reward.data_ptr(), st.done.data_ptr(), W.data_ptr(), clf.data_ptr())
        cached = getattr(self, "_step_args", None)
        if cached is not None and cached[0] == key:
            flags = self._step_flags(learn, apply, interrupt)
            fn = getattr(self.lib, name) if tail else self._step_fn
            _lib.check(fn(self._ctx, *cached[1], C.c_uint32(enabled_mask), C.c_uint64(t), C.c_uint32(flags), self._stream(), *tail),
                       self._ctx, name, self.lib)
            return
        self._chk_operands(st, W, clf)
        flags = self._step_flags(learn, apply, interrupt)
        if st is not getattr(self, "_last_state", None):      # another state object (its memory may be recycled)
            self.invalidate_order()
            self._last_state = st
        ptrs = (_ptr(st.x), _ptr(st.y), _ptr(st.vx), _ptr(st.vy), _ptr(st.option_id), _ptr(st.opt_steps),
                _ptr(st.ep_steps), _ptr(st.qcache), _ptr(st.action), _ptr(st.reward), _ptr(st.done), _ptr(W), _ptr(clf))
        self._step_fn = self.lib.scg_step
        self._step_keep = (st, st.x, st.y, st.vx, st.vy, st.option_id, st.opt_steps, st.ep_steps, st.qcache, st.action,
                           st.reward, st.done, W, clf)    # keeps the ids (and the cached pointers) from being recycled
        self._step_args = (key, ptrs)
        self._call(name, *ptrs, C.c_uint32(enabled_mask), C.c_uint64(t), C.c_uint32(flags), self._stream(), *tail)

    def _chk_record(self, record, N: int, min_rows: int, what: str):
        """The scg_record of a Trajectory whose window lies inside N items, on this device (SPEC §10)."""
        if record.device != self.device:
            raise ScgError(f"{what}: the record is on {record.device}, the context on {self.device}")
        if record.first + record.n > N:
            raise ScgError(f"{what}: record window {record.first}..{record.first + record.n - 1} outside {N} items")
        if record.rows < min_rows:
            raise ScgError(f"{what}: the record has {record.rows} rows, the launch needs {min_rows}")
        self._chk(record.len, torch.int32, record.n, "record.len")
        for f in record.fields:
            self._chk(getattr(record, f), record.DTYPES[f], record.rows * record.n, "record." + f)
        return record.c_struct()

    def _chk_population(self, W: torch.Tensor, population) -> "_lib.Population":
        """The scg_population of rollout(population=(epsilon, enabled[, clf[, gate]])) (SPEC §21): C from W's leading dimension, n_per =
        n_envs // C. (§24.1's clf and §25.1's gate, checked here against that C, are no members of the struct: rollout passes them
        behind it.)"""
        try:
            eps, enabled, *rest = population
            pop_clf, pop_gate = (tuple(rest) + (None, None))[:2] if len(rest) <= 2 else ()
            if len(rest) == 2 and pop_gate is None:            # (the four-element form is for a gate table; three elements say "none")
                raise ValueError
        except (TypeError, ValueError):
            raise ScgError("rollout: population must be (epsilon, enabled) of [C] tensors, either may be None, optionally followed by "
                           "a [C, n_vf, 8] classifier table (or None) and then a [C, n_vf, 2, 5, 1296] gate table") from None
        if not isinstance(W, torch.Tensor) or W.dim() != 4 or tuple(W.shape[1:]) != (self.n_vf, NUM_ACTIONS, NUM_FEATURES):
            raise ScgError(f"rollout: with a population W must be [C, {self.n_vf}, {NUM_ACTIONS}, {NUM_FEATURES}], "
                           f"got {tuple(getattr(W, 'shape', ()))}")
        n_pol = int(W.shape[0])
        if not (1 <= n_pol <= _lib.POP_MAX):
            raise ScgError(f"rollout: a population holds 1 .. {_lib.POP_MAX} policies, W has {n_pol}")
        if self.n_envs % n_pol:
            raise ScgError(f"rollout: {self.n_envs} envs do not divide into {n_pol} policies")
        if eps is not None:
            self._chk(eps, torch.float32, n_pol, "population epsilon")
        if enabled is not None:
            # (the masks fit in a few bits: int32 holds the same words and is what most torch builds can fill and index)
            self._chk(enabled, torch.uint32 if getattr(enabled, "dtype", None) == getattr(torch, "uint32", None) else torch.int32,
                      n_pol, "population enabled")
        if pop_clf is not None:
            if not isinstance(pop_clf, torch.Tensor) or tuple(pop_clf.shape) != (n_pol, self.n_vf, CLF_STRIDE):
                raise ScgError(f"rollout: the population's clf must be [{n_pol}, {self.n_vf}, {CLF_STRIDE}], "
                               f"got {tuple(getattr(pop_clf, 'shape', ()))}")
            self._chk(pop_clf, torch.float32, n_pol * self.n_vf * CLF_STRIDE, "population clf")
        if pop_gate is not None:
            shape = (n_pol, self.n_vf, 2, NUM_ACTIONS, NUM_FEATURES)
            if not isinstance(pop_gate, torch.Tensor) or tuple(pop_gate.shape) != shape:
                raise ScgError(f"rollout: the population's gate must be {list(shape)}, got {tuple(getattr(pop_gate, 'shape', ()))}")
            self._chk(pop_gate, torch.float32, pop_gate.numel(), "population gate")
        return _lib.Population(n_pol, self.n_envs // n_pol, _ptr(eps), _ptr(enabled))

    def rollout(self, st: "EnvState", W: torch.Tensor, clf: torch.Tensor, enabled_mask: int, t0: int, n_steps: int,
                stats=None, begin: bool = False, one_episode: bool = False, record=None, begin_at: bool = False,
                interrupt: bool = False, interrupts=None, choose: Optional[str] = None, overrides=None, audit=None,
                first_action: Optional[torch.Tensor] = None, population=None) -> None:
        """SPEC §8: n_steps acting steps in ONE launch, bit for bit n_steps calls of step(learn=False) at t0 .. t0+n_steps-1
        (with `begin`: a new episode for every env at t0 first, the steps at t0+1 .. t0+n_steps). W is read, never written.
        `stats` (EpisodeStats of this context's n_vf and n_envs, on its device) receives the episode counters; `one_episode`
        leaves envs alone whose `stats.finished` is set. The step's prepared env order is invalid afterwards.
        SPEC §10: `record` (a Trajectory) receives the per-step rows of its window of envs; `begin_at` is `begin` from the
        state in `st` (x, y, vx, vy as given) instead of a drawn start. Neither changes any other output.
        SPEC §11: `interrupt` cuts a running option short wherever max_a Q_0(s', .) exceeds max_a Q_o(s', .) (scg_rollout_interrupt);
        `interrupts` ([n_vf][n_envs] int32, in/out) counts the interrupted steps per option, by default into `stats.interrupts`
        (which then shows in stats.summary()).
        SPEC §14: `choose="value"` offers an env the candidate option of the highest value instead of the lowest-numbered one
        (scg_rollout_select, the only path that goes through it); `overrides` ([n_vf][n_envs] int32, in/out) counts the entries
        of an option that was not the lowest-numbered candidate, by default into `stats.overrides` (created on demand).
        SPEC §15: `audit` (a GateAudit of n_envs envs on this device) makes the launch an audited one (scg_rollout_audit, with the
        rules `interrupt` and `choose` name): its `force`, where set, decides the begin pseudo-step's choice (begin or begin_at
        only), and its arrays receive the begin choice, the values it compared and the discounted task return.
        SPEC §19: `first_action` (uint8 [n_envs] on this device, read only) makes the launch a branch rollout (scg_rollout_branch, with
        whatever else was asked for): on the launch's first real step an env whose entry is below 5 takes that action instead of
        §4.3's choice, the step's draw made as ever; 255 (_lib.NO_FIRST_ACTION) leaves an env alone. It needs n_steps >= 1.
        SPEC §21: `population` = (epsilon, enabled), float32 / int32 (or uint32) [C] tensors on this device, either None (the context's epsilon /
        `enabled_mask` for every policy), makes the launch a population rollout (scg_rollout_population, with whatever else was
        asked for): W is [C, n_vf, 5, 1296], and the envs c * n_per .. (c + 1) * n_per - 1, n_per = n_envs // C, act under W[c],
        epsilon[c] and enabled[c], their draws keyed by the env's index within its range: every policy sees the same start
        states and the same draws, and its range equals by bits a rollout of n_per envs under that policy alone.
        SPEC §24.1: `population` = (epsilon, enabled, clf) with clf a float32 [C, n_vf, 8] tensor on this device (or None) gives
        every policy its own classifier table too (scg_rollout_population_clf): policy c reads clf[c] wherever the rollout reads
        a classifier, and the `clf` argument is then no policy's.
        SPEC §25.1: `population` = (epsilon, enabled, clf, gate) with gate a float32 [C, n_vf, 2, 5, 1296] tensor on this device (no
        gate table: the three-element form) gives every policy a gate table (scg_rollout_population_gate): the value gate of option k compares max_a Q(s_next, .)
        under gate[c][k][0] against the same under gate[c][k][1] and nothing else reads the table; not with `interrupt` or
        `choose="value"`."""
        if choose not in (None, "value"):
            raise ValueError(f"rollout: choose must be None or 'value', not {choose!r}")
        N = self.n_envs
        pop = pop_clf = pop_gate = None
        if population is not None:
            pop = self._chk_population(W, population)
            pop_clf = population[2] if len(population) >= 3 else None
            pop_gate = population[3] if len(population) >= 4 else None
            if pop_gate is not None and (interrupt or choose is not None):
                raise ScgError("rollout: a gate table goes with neither interrupt nor choose='value' (SPEC §25.1)")
        self._chk_operands(st, W, clf, 1 if pop is None else pop.n_policies)
        n_steps, t0 = int(n_steps), int(t0)
        if begin and begin_at:
            raise ScgError("rollout: begin and begin_at together")
        if not (0 <= n_steps <= _lib.ROLLOUT_MAX_STEPS) or (n_steps == 0 and not (begin or begin_at)):
            raise ScgError(f"rollout: n_steps must be in [1, {_lib.ROLLOUT_MAX_STEPS}] ([0, ...] with begin=True)")
        if not (0 <= t0 < 2 ** 64):
            raise ScgError("rollout: t0 must be a 64-bit unsigned step counter")
        cs = None
        if stats is not None:
            if stats.n != N or stats.n_vf != self.n_vf:
                raise ScgError(f"rollout: stats are for {stats.n} envs x {stats.n_vf} VFs, the context has {N} x {self.n_vf}")
            self._chk(stats.ep_return, torch.float32, N, "stats.ep_return"); self._chk(stats.ret_sum, torch.float64, N, "stats.ret_sum")
            for f in ("episodes", "goals", "len_sum"):
                self._chk(getattr(stats, f), torch.int32, N, "stats." + f)
            for f in ("vf_steps", "entries", "declines", "successes"):
                self._chk(getattr(stats, f), torch.int32, self.n_vf * N, "stats." + f)
            self._chk(stats.finished, torch.uint8, N, "stats.finished")
            cs = stats.c_struct()
        elif one_episode:
            raise ScgError("rollout: one_episode needs stats (its `finished` flags)")
        flags = ((_lib.ROLLOUT_BEGIN if begin else 0) | (_lib.ROLLOUT_ONE_EPISODE if one_episode else 0)
                 | (_lib.ROLLOUT_BEGIN_AT if begin_at else 0))
        if interrupts is not None and not interrupt:
            raise ScgError("rollout: interrupts without interrupt=True")
        if interrupt:
            if interrupts is None and stats is not None:
                interrupts = stats.interrupts
            if interrupts is not None:
                self._chk(interrupts, torch.int32, self.n_vf * N, "interrupts")
        if overrides is not None and choose is None:
            raise ScgError("rollout: overrides without choose='value'")
        if choose is not None:
            if overrides is None and stats is not None:
                overrides = stats.want_overrides()
            if overrides is not None:
                self._chk(overrides, torch.int32, self.n_vf * N, "overrides")
        rc = None if record is None else self._chk_record(record, N, n_steps + (1 if begin or begin_at else 0), "rollout")
        au = None
        if audit is not None:
            if audit.n != N or audit.device != self.device:
                raise ScgError(f"rollout: the audit is for {audit.n} envs on {audit.device}, the context has {N} on {self.device}")
            if audit.force is not None and not (begin or begin_at):
                raise ScgError("rollout: audit.force without begin or begin_at")
            for f, dt in audit.DTYPES.items():
                if getattr(audit, f) is not None:
                    self._chk(getattr(audit, f), dt, N, "audit." + f)
            au = audit.c_struct()
        if first_action is not None:
            self._chk(first_action, torch.uint8, N, "first_action")
            if n_steps == 0:
                raise ScgError("rollout: first_action with n_steps = 0: there is no real step to force")
        # the narrowest entry point that takes what was asked for, and its tail behind the arguments all five start with
        rules = (_lib.SELECT_BEST if choose is not None else 0) | (_lib.SELECT_INTERRUPT if interrupt else 0)
        ints, ovr = (None if a is None else _ptr(a) for a in (interrupts, overrides))
        rc_ref = None if rc is None else C.byref(rc)
        if pop is not None:
            name = ("scg_rollout_population_gate" if pop_gate is not None
                    else "scg_rollout_population" if pop_clf is None else "scg_rollout_population_clf")
            tail = (ints, ovr, rc_ref, C.c_uint32(rules), None if au is None else C.byref(au),
                    _ptr(first_action))
        elif first_action is not None:
            name, tail = "scg_rollout_branch", (ints, ovr, rc_ref, C.c_uint32(rules), None if au is None else C.byref(au),
                                                _ptr(first_action))
        elif au is not None:
            name, tail = "scg_rollout_audit", (ints, ovr, rc_ref, C.c_uint32(rules), C.byref(au))
        elif choose is not None:
            name, tail = "scg_rollout_select", (ints, ovr, rc_ref, C.c_uint32(rules))
        elif interrupt:
            name, tail = "scg_rollout_interrupt", (ints, rc_ref)
        elif record is not None or begin_at:
            name, tail = "scg_rollout_record", (rc_ref,)
        else:
            name, tail = "scg_rollout", ()
        self._call(name, _ptr(st.x), _ptr(st.y), _ptr(st.vx), _ptr(st.vy), _ptr(st.option_id), _ptr(st.opt_steps), _ptr(st.ep_steps),
                   _ptr(st.qcache), _ptr(st.action), _ptr(st.reward), _ptr(st.done), _ptr(W), _ptr(clf), C.c_uint32(enabled_mask),
                   C.c_uint64(t0), C.c_int32(n_steps), C.c_uint32(flags), None if cs is None else C.byref(cs), *tail, self._stream(),
                   *(() if pop is None else (C.byref(pop),)),
                   *(() if pop_clf is None and pop_gate is None else (_ptr(pop_clf),)), *(() if pop_gate is None else (_ptr(pop_gate),)))
        if stats is not None and interrupt and interrupts is stats.interrupts:
            stats.interrupting = True

    def option_trials(self, x: torch.Tensor, y: torch.Tensor, vx: torch.Tensor, vy: torch.Tensor, option: torch.Tensor,
                      W: torch.Tensor, clf: torch.Tensor, enabled_mask: int, t0: int, out, record=None) -> None:
        """SPEC §9: entry i runs option option[i] from (x, y, vx, vy)[i] until the option terminates, all in ONE launch, each
        step bit for bit an acting step(learn=False) of an env running that option. `out` (TrialResult of the same length, on
        this device) receives outcome, steps, ret, disc_ret, v0 and the end state; an entry whose option is not known
        (enabled_mask | the gestation mask) is not run (outcome 0). W and clf are read only; nothing else is written.
        `record` (a Trajectory over entries) receives the per-step rows of SPEC §10; it changes no other output."""
        n = x.numel()
        if n < 1:
            raise ScgError("option_trials: need at least one start state")
        x, y, vx, vy = self._chk4((x, y, vx, vy), n, "state")
        self._chk(option, torch.int32, n, "option")
        _chk_W(self, W); _chk_clf(self, clf)
        if out.n != n:
            raise ScgError(f"option_trials: out holds {out.n} entries, the call has {n}")
        self._chk(out.outcome, torch.uint8, n, "out.outcome"); self._chk(out.steps, torch.int32, n, "out.steps")
        for f in out.FIELDS[2:]:
            self._chk(getattr(out, f), torch.float32, n, "out." + f)
        if not (0 <= int(t0) < 2 ** 64):
            raise ScgError("option_trials: t0 must be a 64-bit unsigned step counter")
        cs = out.c_struct()
        head = (C.c_int32(n), _ptr(x), _ptr(y), _ptr(vx), _ptr(vy), _ptr(option), _ptr(W), _ptr(clf), C.c_uint32(enabled_mask),
                C.c_uint64(int(t0)), C.byref(cs))
        if record is None:
            self._call("scg_option_trials", *head, self._stream())
        else:
            rc = self._chk_record(record, n, 1, "option_trials")
            self._call("scg_option_trials_record", *head, C.byref(rc), self._stream())

    def invalidate_order(self) -> None:
        """Tell the library that option ids were written outside scg_step (reset, restore): re-sort next step."""
        self._step_args = self._step_keep = None
        self._call("scg_invalidate_order")

    def set_option_parents(self, parents) -> None:
        """SPEC §4.2 option graph: parents[k] (k = 1..n_options) = option whose initiation set option k targets,
        0 = the task goal. Default is the chain k -> k-1. Validated (range, acyclic) by the library."""
        arr = np.zeros(self.n_options + 1, np.int32)
        arr[1:] = np.asarray(list(parents)[1:self.n_options + 1] if len(parents) > self.n_options
                             else list(parents), np.int32)[: self.n_options]
        self.parents = arr
        self._call("scg_set_option_parents", arr.ctypes.data_as(C.c_void_p))

    # ------------------------------------------------------------------ outer-loop support (SPEC §7)
    def set_trace_buffers(self, ring_len: int):
        """Allocate and attach the trajectory ring + event buffers; returns (ring_x, ring_y, events, ev_len).
        ring_len must be a power of two; ring_len = 0 detaches."""
        self._armed = None                 # the library drops an announced trigger with the buffers it refers to
        if ring_len == 0:
            self._call("scg_set_trace_buffers", None, None, 0, None, None)
            self._trace = None
            return None
        if ring_len < 1 or ring_len & (ring_len - 1):
            raise ScgError("ring_len must be a power of two")
        N = self.n_envs
        ring_x = torch.zeros((ring_len, N), dtype=torch.float32, device=self.device)
        ring_y = torch.zeros((ring_len, N), dtype=torch.float32, device=self.device)
        events = torch.zeros(N, dtype=torch.uint8, device=self.device)
        ev_len = torch.zeros(N, dtype=torch.int32, device=self.device)
        self._call("scg_set_trace_buffers", _ptr(ring_x), _ptr(ring_y), ring_len, _ptr(events), _ptr(ev_len))
        self._trace = (ring_x, ring_y, events, ev_len)
        return self._trace

    def harvest(self, sel_env: torch.Tensor, l_pos: int, l_neg: int):
        """Examples for the listed envs (int32, device) from the ring: (xy[n,L,2] f32, label[n,L] u8)."""
        if self._trace is None:
            raise ScgError("harvest: trace buffers are not attached (set_trace_buffers)")
        ring_x, ring_y, _, ev_len = self._trace
        n = sel_env.numel()
        self._chk(sel_env, torch.int32, n, "sel_env")
        if n and (int(sel_env.min()) < 0 or int(sel_env.max()) >= self.n_envs):
            raise ScgError("harvest: env index out of range")
        L = l_pos + l_neg
        if l_pos < 0 or l_neg < 0 or L < 1:
            raise ScgError("harvest: need l_pos + l_neg >= 1")
        xy = torch.zeros((n, L, 2), dtype=torch.float32, device=self.device)
        lab = torch.zeros((n, L), dtype=torch.uint8, device=self.device)
        self._call("scg_harvest", n, _ptr(sel_env), _ptr(ring_x), _ptr(ring_y), ring_x.shape[0], _ptr(ev_len),
                   l_pos, l_neg, _ptr(xy), _ptr(lab), self._stream())
        return xy, lab

    def collect_examples(self, event_bits: int, prev_in: Optional[torch.Tensor], l_pos: int, l_neg: int,
                         ex_xy: torch.Tensor, ex_label: torch.Tensor, count: torch.Tensor, rearm: bool = True) -> None:
        """SPEC §7 device-side trigger: envs whose events byte has one of `event_bits` set (with prev_in: on the step the
        bit goes up) append their most recent ring states to ex_xy[cap, 2] / ex_label[cap] behind the count[0] examples
        already there (device int32[1], in/out). Two small launches (row totals, then prefix + gather) — one when the
        trigger was announced (`rearm`, scg_arm_collect: the step's own commit rows then leave the row totals); nothing
        comes back to the host. With `rearm` the library keeps the RAW device pointers of prev_in and count and reads
        them inside every later scg_step until disarm_collect() / set_trace_buffers(): this object holds references to
        both tensors for exactly that long, so dropping yours cannot leave the step reading freed memory."""
        if self._trace is None:
            raise ScgError("collect_examples: trace buffers are not attached (set_trace_buffers)")
        cap = ex_label.numel()
        self._chk(ex_xy, torch.float32, 2 * cap, "ex_xy"); self._chk(ex_label, torch.uint8, cap, "ex_label")
        self._chk(count, torch.int32, 1, "count")
        if prev_in is not None:
            self._chk(prev_in, torch.uint8, self.n_envs, "prev_in")
        if l_pos < 0 or l_neg < 0 or l_pos + l_neg < 1 or not (0 < event_bits < 64):
            raise ScgError("collect_examples: bad argument")
        self._call("scg_collect_examples", C.c_uint32(event_bits), _ptr(prev_in), l_pos, l_neg, _ptr(ex_xy), _ptr(ex_label),
                   _ptr(count), cap, self._stream())
        if rearm:            # the same trigger will come again after the next step: let that step leave the row totals behind
            self._call("scg_arm_collect", C.c_uint32(event_bits), _ptr(prev_in), l_pos, l_neg, _ptr(count))
            self._armed = (prev_in, count)       # keeps the announced buffers alive while the library holds their addresses
        else:
            self.disarm_collect()

    def collect_frontier(self, target_mask: int, cover_mask: int, clf: torch.Tensor, l_pos: int, l_neg: int,
                         ex_xy: torch.Tensor, ex_label: torch.Tensor, count: torch.Tensor) -> None:
        """SPEC §13 frontier collection, one buffer per node p = 0..n_options (0 = the goal, p = initiation set p): an env
        whose step ended in a node of `target_mask` while its s_t lay in no initiation set of `cover_mask` (classifier rows
        of clf[n_vf, 8]) appends its most recent ring states to ex_xy[n_vf, cap, 2] / ex_label[n_vf, cap] behind count[p]
        (device int32[n_vf], in/out). Two small launches; stateless (no prev_in, an announced collect_examples trigger is
        left alone); nothing comes back to the host."""
        if self._trace is None:
            raise ScgError("collect_frontier: trace buffers are not attached (set_trace_buffers)")
        cap = ex_label.numel() // self.n_vf
        if cap < 1 or ex_label.numel() != self.n_vf * cap:
            raise ScgError(f"collect_frontier: ex_label must hold n_vf = {self.n_vf} buffers of cap >= 1 examples")
        self._chk(ex_xy, torch.float32, 2 * self.n_vf * cap, "ex_xy"); self._chk(ex_label, torch.uint8, self.n_vf * cap, "ex_label")
        self._chk(count, torch.int32, self.n_vf, "count"); _chk_clf(self, clf)
        nodes = (1 << self.n_vf) - 1
        if l_pos < 0 or l_neg < 0 or l_pos + l_neg < 1 or not (0 <= target_mask <= nodes) or not (0 <= cover_mask <= nodes) \
                or cover_mask & 1 or target_mask & ~cover_mask & ~1:
            raise ScgError("collect_frontier: bad argument")
        self._call("scg_collect_frontier", C.c_uint32(target_mask), C.c_uint32(cover_mask), _ptr(clf), l_pos, l_neg, _ptr(ex_xy),
                   _ptr(ex_label), _ptr(count), cap, self._stream())

    def disarm_collect(self) -> None:
        self._call("scg_arm_collect", C.c_uint32(0), None, 0, 0, None)
        self._armed = None

    def set_gestation(self, gest_mask: int, counters: bool = True) -> Optional[torch.Tensor]:
        """SPEC §4.4: options in gestation (known, never selected, learning off-policy). Returns the device int32[n_vf] success
        counters the fused step adds to (kept across calls; zero an entry when its option starts gestating); with counters=False
        the classifiers are in use but no counts are kept (a context that only acts) and None is returned."""
        if counters and self._gest_succ is None:
            self._gest_succ = torch.zeros(self.n_vf, dtype=torch.int32, device=self.device)
        succ = self._gest_succ if counters else None
        self._call("scg_set_gestation", C.c_uint32(gest_mask), _ptr(succ))
        self.gest_mask = gest_mask
        return succ

    def grad_buffers(self):
        """(G[n_vf,5,1296] float32, n_k[n_vf] int32): caller-owned torch tensors that scg_step(LEARN)
        fills with the rank-local gradient sum and update counts (the all-reduce operands, SPEC §5)."""
        if self._gbuf is None:
            G = torch.zeros((self.n_vf, NUM_ACTIONS, NUM_FEATURES), dtype=torch.float32, device=self.device)
            n = torch.zeros((self.n_vf,), dtype=torch.int32, device=self.device)
            self._call("scg_set_grad_buffers", _ptr(G), _ptr(n))
            self._gbuf, self._gpacked = (G, n), None
        return self._gbuf

    def grad_packed(self) -> torch.Tensor:
        """One flat float32 tensor [n_vf*5*1296 + n_vf]: G followed by the update counts as floats — the single
        all-reduce operand of a sharded run with shared weights (scg_set_grad_buffer_packed)."""
        if self._gpacked is None:
            gp = torch.zeros(self.n_vf * (W_ROW + 1), dtype=torch.float32, device=self.device)
            self._call("scg_set_grad_buffer_packed", _ptr(gp))
            self._gpacked, self._gbuf = gp, None
        return self._gpacked

    def apply_update_packed(self, W: torch.Tensor, gp: torch.Tensor) -> None:
        _chk_W(self, W); _chk_packed(self, gp, "G_packed")
        self._call("scg_apply_update_packed", _ptr(W), _ptr(gp), self._stream())

    def apply_update_slots(self, W: torch.Tensor, slots: torch.Tensor) -> None:
        """The order-pinned multi-rank update (SPEC §5): `slots` [n_ranks, n_vf*5*1296 + n_vf] holds every rank's packed operand
        (an all-gather of grad_packed()); G and the counts are summed in slot order: the weights are identical on every rank of a run and reproducible by the oracle for any number of ranks (the rank count, like the block size and the seed, is part of the run's identity)."""
        per = self.n_vf * (W_ROW + 1)
        if slots.dim() != 2 or slots.shape[1] != per or not slots.is_contiguous():
            raise ScgError(f"slots must be a contiguous [n_ranks, {per}] tensor")
        _chk_W(self, W); _chk_packed(self, slots, "slots", slots.shape[0])
        self._call("scg_apply_update_slots", _ptr(W), _ptr(slots), C.c_int32(slots.shape[0]), C.c_int64(per), self._stream())

    def apply_update(self, W: torch.Tensor, G: torch.Tensor, n_k: torch.Tensor) -> None:
        _chk_W(self, W); _chk_W(self, G, "G")
        self._chk(n_k, torch.int32, self.n_vf, "n_k")
        self._call("scg_apply_update", _ptr(W), _ptr(G), _ptr(n_k), self._stream())

    # ------------------------------------------------------------------ un-fused entry points
    def _chk4(self, s: Sequence[torch.Tensor], n: int, name: str):
        if len(s) != 4:
            raise ScgError(f"{name}: need (x, y, vx, vy)")
        return [self._chk(t, torch.float32, n, f"{name}[{i}]") for i, t in enumerate(s)]

    def pinball_step(self, s, action: torch.Tensor):
        n = s[0].numel()
        x, y, vx, vy = self._chk4(s, n, "state")
        self._chk(action, torch.uint8, n, "action")
        if n and int(action.max()) >= NUM_ACTIONS:
            raise ScgError("action out of range [0, 5)")
        reward = torch.empty(n, dtype=torch.float32, device=self.device)
        goal = torch.empty(n, dtype=torch.uint8, device=self.device)
        self._call("scg_pinball_step", n, _ptr(x), _ptr(y), _ptr(vx), _ptr(vy), _ptr(action), _ptr(reward),
                   _ptr(goal), self._stream())
        return reward, goal

    def features(self, s) -> torch.Tensor:
        n = s[0].numel()
        x, y, vx, vy = self._chk4(s, n, "state")
        phi = torch.empty((n, NUM_FEATURES), dtype=torch.float32, device=self.device)
        self._call("scg_fourier_features", n, _ptr(x), _ptr(y), _ptr(vx), _ptr(vy), _ptr(phi), self._stream())
        return phi

    def _gram_setup(self, fn: str, offsets, *states, features: int = NUM_FEATURES):
        """What feature_gram, feature_cross_gram and basis_gram (`fn`) share: the checked state tensors of each of `states`
        (placeholders when n = 0), n, the offsets as a host int64 array, n_seg and the uninitialised output [n_seg][F][F], F =
        `features` (1296 but for basis_gram)."""
        n = states[0][0].numel()
        sv = [self._chk4(s, n, name) for s, name in zip(states, ("state", "successor state"))]
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
        n_seg = len(off) - 1
        if not (1 <= n_seg <= _lib.GRAM_MAX_SEGMENTS):
            raise ScgError(f"{fn}: offsets must name 1 .. {_lib.GRAM_MAX_SEGMENTS} segments")
        if off[0] < 0 or off[-1] > n or np.any(np.diff(off) < 0):
            raise ScgError(f"{fn}: offsets must be non-decreasing and inside [0, n]")
        if n == 0:                                           # (an empty tensor has no address: the entry point refuses a null array)
            sv = [[torch.zeros(1, dtype=torch.float32, device=self.device)] * 4] * len(sv)
        out = torch.empty((n_seg, features, features), dtype=torch.float32, device=self.device)
        return sv, n, off, n_seg, out

    def feature_gram(self, s, offsets, yv: Optional[torch.Tensor] = None):
        """SPEC §16.1: A[g] = sum phi(s_n) phi(s_n)^T over segment g = samples offsets[g] .. offsets[g+1]-1 of the states `s`
        (`offsets`: host integers, non-decreasing, inside [0, n]); with `yv` [n] also b[g] = sum phi(s_n) yv[n]. Returns A
        [n_seg][1296][1296], or (A, b [n_seg][1296]). phi is not materialised; the sums have §16.1's pinned order."""
        (a,), n, off, n_seg, A = self._gram_setup("feature_gram", offsets, s)
        if yv is not None:
            self._chk(yv, torch.float32, n, "yv")
            yv = yv if n else a[0]
        b = None if yv is None else torch.empty((n_seg, NUM_FEATURES), dtype=torch.float32, device=self.device)
        self._call("scg_feature_gram", C.c_int64(n), *[_ptr(t) for t in a], _ptr(yv), n_seg,
                   off.ctypes.data_as(C.c_void_p), _ptr(A), _ptr(b), self._stream())
        return A if b is None else (A, b)

    def feature_gram_targets(self, s, offsets, Y: torch.Tensor):
        """SPEC §20.1: feature_gram's A and, for the targets `Y` (a contiguous float32 [n_tgt][n], 1 <= n_tgt <= 16), B[g][c] = sum
        phi(s_n) Y[c][n] over segment g: one Gram, a right-hand side per target, for the MFMAs one right-hand side costs. Returns
        (A [n_seg][1296][1296], B [n_seg][n_tgt][1296]); A and every B[g][c] have the bits feature_gram gives for yv = Y[c]."""
        (a,), n, off, n_seg, A = self._gram_setup("feature_gram_targets", offsets, s)
        if not isinstance(Y, torch.Tensor) or Y.dim() != 2 or not (1 <= Y.shape[0] <= _lib.GRAM_MAX_TARGETS) or Y.shape[1] != n:
            raise ScgError(f"feature_gram_targets: Y must be [n_tgt][{n}] with 1 <= n_tgt <= {_lib.GRAM_MAX_TARGETS}")
        n_tgt = int(Y.shape[0])
        self._chk(Y, torch.float32, n_tgt * n, "Y")
        Y = Y if n else a[0]
        B = torch.empty((n_seg, n_tgt, NUM_FEATURES), dtype=torch.float32, device=self.device)
        self._call("scg_feature_gram_targets", C.c_int64(n), *[_ptr(t) for t in a], _ptr(Y), n_tgt, n_seg,
                   off.ctypes.data_as(C.c_void_p), _ptr(A), _ptr(B), self._stream())
        return A, B

    def feature_gram_weighted(self, s, offsets, root_weights: torch.Tensor, Y: Optional[torch.Tensor] = None):
        """SPEC §22.1: feature_gram_targets with a root weight per sample on every operand: A[g] = sum u(n) u(n)^T and B[g][c] = sum
        u(n) t_c(n) over segment g, u(n) = root_weights[n] * phi(s_n) and t_c(n) = root_weights[n] * Y[c][n], one binary32 multiply
        each: the weighted normal equations with the weights root_weights^2 (valuefit.root_weights gives the roots). `root_weights`
        a contiguous float32 [n]; `Y` a contiguous float32 [n_tgt][n], 1 <= n_tgt <= 16, or None. Returns (A [n_seg][1296][1296],
        B [n_seg][n_tgt][1296] or None); unit weights give feature_gram_targets' bits."""
        (a,), n, off, n_seg, A = self._gram_setup("feature_gram_weighted", offsets, s)
        self._chk(root_weights, torch.float32, n, "root_weights")
        rw = root_weights if n else a[0]
        n_tgt, B = 0, None
        if Y is not None:
            if not isinstance(Y, torch.Tensor) or Y.dim() != 2 or not (1 <= Y.shape[0] <= _lib.GRAM_MAX_TARGETS) or Y.shape[1] != n:
                raise ScgError(f"feature_gram_weighted: Y must be [n_tgt][{n}] with 1 <= n_tgt <= {_lib.GRAM_MAX_TARGETS}")
            n_tgt = int(Y.shape[0])
            self._chk(Y, torch.float32, n_tgt * n, "Y")
            Y = Y if n else a[0]
            B = torch.empty((n_seg, n_tgt, NUM_FEATURES), dtype=torch.float32, device=self.device)
        self._call("scg_feature_gram_weighted", C.c_int64(n), *[_ptr(t) for t in a], _ptr(rw), _ptr(Y), n_tgt, n_seg,
                   off.ctypes.data_as(C.c_void_p), _ptr(A), _ptr(B), self._stream())
        return A, B

    def feature_cross_gram(self, s, s2, offsets):
        """SPEC §17.1: C[g] = sum phi(s_n) phi(s2_n)^T over segment g = samples offsets[g] .. offsets[g+1]-1 of the state pairs
        (`s`, `s2`: four [n] tensors each, which may be the same tensors; `offsets` as for feature_gram). Returns C
        [n_seg][1296][1296]: rows the features of s, columns those of s2. phi is not materialised; the sums have §16.1's pinned order."""
        (a, b), n, off, n_seg, Cm = self._gram_setup("feature_cross_gram", offsets, s, s2)
        self._call("scg_feature_cross_gram", C.c_int64(n), *[_ptr(t) for t in a], *[_ptr(t) for t in b], n_seg,
                   off.ctypes.data_as(C.c_void_p), _ptr(Cm), self._stream())
        return Cm

    # SPEC §18, the basis-order probe: the basis of order p in _lib.BASIS_ORDERS, F = (p + 1)^4 features
    def basis_features(self, order: int, s) -> torch.Tensor:
        """phi [n][F] of order `order`; at order 5 features()' bits."""
        F = _lib.basis_features(order)
        n = s[0].numel()
        x, y, vx, vy = self._chk4(s, n, "state")
        phi = torch.empty((n, F), dtype=torch.float32, device=self.device)
        self._call("scg_basis_features", int(order), C.c_int64(n), _ptr(x), _ptr(y), _ptr(vx), _ptr(vy), _ptr(phi), self._stream())
        return phi

    def basis_gram(self, order: int, s, offsets, yv: Optional[torch.Tensor] = None):
        """feature_gram at order `order`: A [n_seg][F][F], or (A, b [n_seg][F]) with `yv`; SPEC §16.1's pinned order with 1296 -> F.
        At order 5 feature_gram's bits; the A and b of a lower order are the sub-block at the embedded indices, by bits."""
        F = _lib.basis_features(order)
        (a,), n, off, n_seg, A = self._gram_setup("basis_gram", offsets, s, features=F)
        if yv is not None:
            self._chk(yv, torch.float32, n, "yv")
            yv = yv if n else a[0]
        b = None if yv is None else torch.empty((n_seg, F), dtype=torch.float32, device=self.device)
        self._call("scg_basis_gram", int(order), C.c_int64(n), *[_ptr(t) for t in a], _ptr(yv), n_seg,
                   off.ctypes.data_as(C.c_void_p), _ptr(A), _ptr(b), self._stream())
        return A if b is None else (A, b)

    def basis_values(self, order: int, s, V: torch.Tensor) -> torch.Tensor:
        """out [m][n] = sum_f V[r][f] phi_f(s_n) for the rows of V [m][F], 1 <= m <= 8, in SPEC §18.3's pinned order (not q_values'
        order, also at order 5)."""
        F = _lib.basis_features(order)
        n = s[0].numel()
        x, y, vx, vy = self._chk4(s, n, "state")
        if not isinstance(V, torch.Tensor) or V.dim() != 2 or not (1 <= V.shape[0] <= _lib.BASIS_VALUES_MAX_ROWS):
            raise ScgError(f"basis_values: V must be [m][{F}] with 1 <= m <= {_lib.BASIS_VALUES_MAX_ROWS}")
        m = int(V.shape[0])
        self._chk(V, torch.float32, m * F, "V")
        out = torch.empty((m, n), dtype=torch.float32, device=self.device)
        self._call("scg_basis_values", int(order), C.c_int64(n), _ptr(x), _ptr(y), _ptr(vx), _ptr(vy), _ptr(V), m, _ptr(out),
                   self._stream())
        return out

    # SPEC §23, the instruments of initfit.irls_fit
    def logistic_terms(self, z: torch.Tensor, label: torch.Tensor):
        """SPEC §23.1: (p, rw, e) float32 [n] from the logits `z` (float32 [n]) and the labels `label` (uint8 [n], non-zero is 1):
        p = SPEC §6's sigmoid, e = l - p, rw = sqrt(p (1 - p)), one binary32 operation each."""
        if not isinstance(z, torch.Tensor) or z.dim() != 1:
            raise ScgError("logistic_terms: z must be a float32 [n] tensor")
        n = z.numel()
        self._chk(z, torch.float32, n, "z")
        self._chk(label, torch.uint8, n, "label")
        p, rw, e = (torch.empty(n, dtype=torch.float32, device=self.device) for _ in range(3))
        if n:                                                # (an empty tensor has no address; n = 0 writes nothing)
            self._call("scg_logistic_terms", C.c_int64(n), _ptr(z), _ptr(label), _ptr(p), _ptr(rw), _ptr(e), self._stream())
        return p, rw, e

    def basis_gram_irls(self, order: int, s, offsets, rw: torch.Tensor, e: torch.Tensor):
        """SPEC §23.2: (H [n_seg][F][F], grad [n_seg][F]) at order `order`: H[g] = sum u(n) u(n)^T with u(n) = rw[n] * phi(s_n), the
        weighted Gram of feature_gram_weighted at the order's phi, and grad[g] = sum phi(s_n) e[n] with the UNWEIGHTED phi,
        basis_gram's b for yv = e. `rw`, `e`: contiguous float32 [n] (logistic_terms gives both)."""
        F = _lib.basis_features(order)
        (a,), n, off, n_seg, H = self._gram_setup("basis_gram_irls", offsets, s, features=F)
        self._chk(rw, torch.float32, n, "rw")
        self._chk(e, torch.float32, n, "e")
        rw, e = (rw, e) if n else (a[0], a[0])
        grad = torch.empty((n_seg, F), dtype=torch.float32, device=self.device)
        self._call("scg_basis_gram_irls", int(order), C.c_int64(n), *[_ptr(t) for t in a], _ptr(rw), _ptr(e), n_seg,
                   off.ctypes.data_as(C.c_void_p), _ptr(H), _ptr(grad), self._stream())
        return H, grad

    def ridge_solve(self, A: torch.Tensor, B: torch.Tensor, lam: torch.Tensor, mu, skip=None):
        """SPEC §31: the pinned-order ridge solve on the device. `A` float32 [n_mat][F][F] as the Gram calls leave it (its lower
        triangle is read), `B` float32 [n_mat][n_rhs][F] or [n_mat][F], `lam` float64 [F] on the device, `mu` host floats [n_mat]
        (M_ii = A_ii + mu[g] * lam[i]), `skip` host flags [n_mat] (None: none). F a multiple of 16 up to 4096, n_mat <= 64, n_rhs <=
        16. Returns device tensors (Delta float64 of B's shape, L float64 [n_mat][F][F] — the factor in the lower triangle, the strict
        upper triangle unspecified —, info int32 [n_mat]: 0, or j + 1 for a failed pivot of column j, whose Delta is +0). A skipped
        matrix gets Delta = +0 and info = 0; its L is not written. Nothing is read back."""
        if not isinstance(A, torch.Tensor) or A.dim() != 3 or A.shape[1] != A.shape[2]:
            raise ScgError("ridge_solve: A must be [n_mat][F][F]")
        n_mat, F = int(A.shape[0]), int(A.shape[1])
        if F < 1 or F % _lib.RIDGE_TILE or F > _lib.RIDGE_MAX_F:
            raise ScgError(f"ridge_solve: F must be a positive multiple of {_lib.RIDGE_TILE} up to {_lib.RIDGE_MAX_F}")
        if not (1 <= n_mat <= _lib.GRAM_MAX_SEGMENTS):
            raise ScgError(f"ridge_solve: 1 .. {_lib.GRAM_MAX_SEGMENTS} matrices")
        if not isinstance(B, torch.Tensor) or B.dim() not in (2, 3) or B.shape[0] != n_mat or B.shape[-1] != F:
            raise ScgError(f"ridge_solve: B must be [{n_mat}][n_rhs][{F}] or [{n_mat}][{F}]")
        n_rhs = int(B.shape[1]) if B.dim() == 3 else 1
        if not (1 <= n_rhs <= _lib.GRAM_MAX_TARGETS):
            raise ScgError(f"ridge_solve: 1 .. {_lib.GRAM_MAX_TARGETS} right-hand sides per matrix")
        self._chk(A, torch.float32, n_mat * F * F, "A")
        self._chk(B, torch.float32, n_mat * n_rhs * F, "B")
        self._chk(lam, torch.float64, F, "lam")
        mu = np.ascontiguousarray(np.asarray(mu, dtype=np.float64).reshape(-1))
        skip = np.zeros(n_mat, np.uint8) if skip is None else np.ascontiguousarray((np.asarray(skip).reshape(-1) != 0).astype(np.uint8))
        if len(mu) != n_mat or len(skip) != n_mat:
            raise ScgError(f"ridge_solve: mu and skip must hold {n_mat} entries")
        L = torch.empty((n_mat, F, F), dtype=torch.float64, device=self.device)
        delta = torch.empty(tuple(B.shape), dtype=torch.float64, device=self.device)
        info = torch.empty(n_mat, dtype=torch.int32, device=self.device)
        self._call("scg_ridge_solve", F, n_mat, n_rhs, _ptr(A), _ptr(B), _ptr(lam), mu.ctypes.data_as(C.c_void_p),
                   skip.ctypes.data_as(C.c_void_p), _ptr(L), _ptr(delta), _ptr(info), self._stream())
        return delta, L, info

    def q_values(self, s, Wk: torch.Tensor) -> torch.Tensor:
        n = s[0].numel()
        x, y, vx, vy = self._chk4(s, n, "state")
        self._chk(Wk, torch.float32, NUM_ACTIONS * NUM_FEATURES, "Wk")
        q = torch.empty((NUM_ACTIONS, n), dtype=torch.float32, device=self.device)
        self._call("scg_q_values", n, _ptr(x), _ptr(y), _ptr(vx), _ptr(vy), _ptr(Wk), _ptr(q), self._stream())
        return q

    # SPEC §27, the instruments of valuefit.lambda_targets
    def row_values(self, s, tab: torch.Tensor, W: torch.Tensor, actions: bool = True):
        """SPEC §27.1: (v float32 [n], a uint8 [n] or None) with v[i] = max_a Q_{tab[i]}(s_i, a) under the tables W [n_tab][5][1296]
        (n_tab = W.shape[0] in 1 .. n_vf), the bits of q_values followed by valuefit.greedy_max, and a[i] the lowest index that
        attains it. A row whose `tab` (uint8 [n]) is ROW_NONE or >= n_tab gets v = +0, a = 255; its state is not read. Any n."""
        n = s[0].numel()
        x, y, vx, vy = self._chk4(s, n, "state")
        self._chk(tab, torch.uint8, n, "tab")
        if not isinstance(W, torch.Tensor) or W.dim() != 3 or tuple(W.shape[1:]) != (NUM_ACTIONS, NUM_FEATURES) \
                or not (1 <= W.shape[0] <= self.n_vf):
            raise ScgError(f"row_values: W must be [n_tab][{NUM_ACTIONS}][{NUM_FEATURES}] with 1 <= n_tab <= {self.n_vf}")
        n_tab = int(W.shape[0])
        self._chk(W, torch.float32, n_tab * W_ROW, "W")
        v = torch.empty(n, dtype=torch.float32, device=self.device)
        a = torch.empty(n, dtype=torch.uint8, device=self.device) if actions else None
        if n:                                                # (an empty tensor has no address; n = 0 writes nothing)
            self._call("scg_row_values", C.c_int64(n), _ptr(x), _ptr(y), _ptr(vx), _ptr(vy), _ptr(tab), _ptr(W), n_tab, _ptr(v), _ptr(a),
                       self._stream())
        return v, a

    # SPEC §29, the instruments of valuefit.double_targets
    def _cross_call(self, name: str, s, tab, W_sel, W_val, act, want_a: bool, want_vs: bool):
        """row_values' argument checks on the operands of scg_row_values_cross, then the call: (v, a or None, vs or None)."""
        n = s[0].numel()
        x, y, vx, vy = self._chk4(s, n, "state")
        self._chk(tab, torch.uint8, n, "tab")
        if W_val is None:
            raise ScgError(f"{name}: the valuing tables must be a float32 [n_tab][{NUM_ACTIONS}][{NUM_FEATURES}] tensor")
        n_tab = None
        for W in (W_sel, W_val):
            if W is None:                                    # (W_sel in the given mode: not read)
                continue
            if not isinstance(W, torch.Tensor) or W.dim() != 3 or tuple(W.shape[1:]) != (NUM_ACTIONS, NUM_FEATURES) \
                    or not (1 <= W.shape[0] <= self.n_vf) or (n_tab is not None and int(W.shape[0]) != n_tab):
                raise ScgError(f"{name}: the tables must be [n_tab][{NUM_ACTIONS}][{NUM_FEATURES}] with 1 <= n_tab <= {self.n_vf}, "
                               "the same n_tab for both")
            n_tab = int(W.shape[0])
            self._chk(W, torch.float32, n_tab * W_ROW, "W")
        if act is not None:
            self._chk(act, torch.uint8, n, "act")
        v = torch.empty(n, dtype=torch.float32, device=self.device)
        a = torch.empty(n, dtype=torch.uint8, device=self.device) if want_a else None
        vs = torch.empty(n, dtype=torch.float32, device=self.device) if want_vs else None
        if n:                                                # (an empty tensor has no address; n = 0 writes nothing)
            self._call("scg_row_values_cross", C.c_int64(n), _ptr(x), _ptr(y), _ptr(vx), _ptr(vy), _ptr(tab), _ptr(W_sel), _ptr(W_val),
                       n_tab, _ptr(act), C.c_uint32(_lib.CROSS_GIVEN if act is not None else 0), _ptr(v), _ptr(a), _ptr(vs),
                       self._stream())
        return v, a, vs

    def row_values_cross(self, s, tab: torch.Tensor, W_sel: torch.Tensor, W_val: torch.Tensor, actions: bool = True,
                         sel_values: bool = False):
        """SPEC §29.1: (v float32 [n], a uint8 [n] or None, vs float32 [n] or None). Under the tables W_sel and W_val ([n_tab][5][1296]
        each) a[i] is the lowest index of max_a Q^sel_{tab[i]}(s_i, a), vs[i] that maximum and v[i] = Q^val_{tab[i]}(s_i, a[i]): the
        valuing table's entry at the selecting table's argmax, each Q with the bits of q_values. With W_val = W_sel, (v, a) is
        row_values' by bits and vs = v. A row whose `tab` is ROW_NONE or >= n_tab gets v = +0, a = 255, vs = +0. Any n."""
        if W_sel is None:
            raise ScgError(f"row_values_cross: the selecting tables must be a float32 [n_tab][{NUM_ACTIONS}][{NUM_FEATURES}] tensor")
        return self._cross_call("row_values_cross", s, tab, W_sel, W_val, None, actions, sel_values)

    def row_action_values(self, s, tab: torch.Tensor, W: torch.Tensor, act: torch.Tensor) -> torch.Tensor:
        """SPEC §29.1's given mode: v float32 [n] with v[i] = Q_{tab[i]}(s_i, act[i]) under the tables W [n_tab][5][1296], the bits of
        q_values(W[tab[i]])[act[i]]. `act`: uint8 [n]; a row with act[i] >= 5 or without a table gets +0. Any n."""
        if act is None:
            raise ScgError("row_action_values: act must be a uint8 [n] tensor")
        return self._cross_call("row_action_values", s, tab, None, W, act, False, False)[0]

    def lambda_returns(self, offsets: torch.Tensor, reward: torch.Tensor, done: torch.Tensor, vf: torch.Tensor, term: torch.Tensor,
                       v0: torch.Tensor, vk: torch.Tensor, gamma: float, lam: float, r_option_success: float):
        """SPEC §27.2: (y0, yk) float64 [total], the root and the option stream of the lambda-return over a record in (env, row)
        order. `offsets`: int64 [n_env + 1] ON THE DEVICE (the kernel clamps them into [0, total]); reward, v0, vk float32 [total];
        done, vf, term uint8 [total]. Rows no env owns keep +0."""
        if not isinstance(offsets, torch.Tensor) or offsets.dim() != 1 or offsets.numel() < 1:
            raise ScgError("lambda_returns: offsets must be an int64 [n_env + 1] tensor on the device")
        n_env, total = offsets.numel() - 1, reward.numel()
        self._chk(offsets, torch.int64, n_env + 1, "offsets")
        for t, name in ((reward, "reward"), (v0, "v0"), (vk, "vk")):
            self._chk(t, torch.float32, total, name)
        for t, name in ((done, "done"), (vf, "vf"), (term, "term")):
            self._chk(t, torch.uint8, total, name)
        if not (0.0 <= float(gamma) <= 1.0) or not (0.0 <= float(lam) <= 1.0):
            raise ScgError("lambda_returns: gamma and lam must lie in [0, 1]")
        y0 = torch.zeros(total, dtype=torch.float64, device=self.device)
        yk = torch.zeros(total, dtype=torch.float64, device=self.device)
        if n_env and total:                                  # (an empty tensor has no address)
            self._call("scg_lambda_returns", n_env, _ptr(offsets), C.c_int64(total), _ptr(reward), _ptr(done), _ptr(vf), _ptr(term),
                       _ptr(v0), _ptr(vk), C.c_double(gamma), C.c_double(lam), C.c_double(r_option_success), _ptr(y0), _ptr(yk),
                       self._stream())
        return y0, yk

    def trace_returns(self, offsets: torch.Tensor, reward: torch.Tensor, done: torch.Tensor, vf: torch.Tensor, term: torch.Tensor,
                      action: torch.Tensor, ag: torch.Tensor, v0: torch.Tensor, vk: torch.Tensor, gamma: float, lam,
                      r_option_success: float, cut: bool = True, horizon: bool = False):
        """SPEC §28.1: (y0, yk, h or None) float64 [total], lambda_returns' two streams with a trace coefficient per row: a row
        carries lam[its vf] (`lam`: a float, or a sequence of 1 .. n_vf floats; a vf beyond it reads lam[0]), and with `cut` +0 where
        its recorded `action` is not `ag` of the row before it (uint8 [total] both; ag: the greedy action at a row's state of the
        table that acts on the next row, 255 for none). `horizon` adds h, the root stream's effective length. The other arguments
        are lambda_returns'. Rows no env owns keep +0."""
        if not isinstance(offsets, torch.Tensor) or offsets.dim() != 1 or offsets.numel() < 1:
            raise ScgError("trace_returns: offsets must be an int64 [n_env + 1] tensor on the device")
        n_env, total = offsets.numel() - 1, reward.numel()
        self._chk(offsets, torch.int64, n_env + 1, "offsets")
        for t, name in ((reward, "reward"), (v0, "v0"), (vk, "vk")):
            self._chk(t, torch.float32, total, name)
        for t, name in ((done, "done"), (vf, "vf"), (term, "term"), (action, "action"), (ag, "ag")):
            self._chk(t, torch.uint8, total, name)
        lam_vf = [float(lam)] if np.ndim(lam) == 0 else [float(v) for v in lam]
        if not (1 <= len(lam_vf) <= self.n_vf):
            raise ScgError(f"trace_returns: lam must be a float or a sequence of 1 .. {self.n_vf} floats")
        if not (0.0 <= float(gamma) <= 1.0) or not all(0.0 <= v <= 1.0 for v in lam_vf):
            raise ScgError("trace_returns: gamma and every lam must lie in [0, 1]")
        y0 = torch.zeros(total, dtype=torch.float64, device=self.device)
        yk = torch.zeros(total, dtype=torch.float64, device=self.device)
        h = torch.zeros(total, dtype=torch.float64, device=self.device) if horizon else None
        if n_env and total:                                  # (an empty tensor has no address)
            self._call("scg_trace_returns", n_env, _ptr(offsets), C.c_int64(total), _ptr(reward), _ptr(done), _ptr(vf), _ptr(term),
                       _ptr(action), _ptr(ag), _ptr(v0), _ptr(vk), C.c_double(gamma), (C.c_double * len(lam_vf))(*lam_vf), len(lam_vf),
                       C.c_uint32(_lib.TRACE_CUT if cut else 0), C.c_double(r_option_success), _ptr(y0), _ptr(yk), _ptr(h),
                       self._stream())
        return y0, yk, h

    # SPEC §30.1, the calls of trajectory.DeviceRecord (which owns the tensors and checks their shapes)
    def record_append(self, launch, store, cap: int) -> None:
        """One launch's rows behind the store's earlier ones: `launch` a _lib.Record of the launch buffers, `store` a
        _lib.RecordStore of [n][cap] arrays (both of device pointers whose tensors the caller keeps alive). No sync, no download."""
        self._call("scg_record_append", C.byref(launch), C.byref(store), int(cap), self._stream())

    def record_offsets(self, have: torch.Tensor) -> torch.Tensor:
        """The exclusive scan of `have` (int32 [n]) as int64 [n + 1] on the device."""
        n = have.numel()
        self._chk(have, torch.int32, n, "have")
        off = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        self._call("scg_record_offsets", n, _ptr(have if n else None), _ptr(off), self._stream())
        return off

    def record_pack(self, n: int, cap: int, store, offsets: torch.Tensor, total: int, flat: dict, extra: dict) -> None:
        """The store's rows into the flat (env, row) arrays `flat` (field name -> [total] tensor) and the optional outputs `extra`
        (env, row: int32; tab0, tabk, tabA: uint8; each [total]), all allocated by the caller on this device."""
        self._chk(offsets, torch.int64, int(n) + 1, "offsets")
        fields = ("x", "y", "vx", "vy", "reward", "action", "done", "vf", "term", "option_id")
        for name, t in list(flat.items()) + list(extra.items()):
            if t.device != self.device or not t.is_contiguous() or t.numel() != int(total):
                raise ScgError(f"record_pack: {name} must be a contiguous [{int(total)}] tensor on {self.device}")
        if total:                                            # (an empty tensor has no address; total = 0 writes nothing)
            self._call("scg_record_pack", int(n), int(cap), C.byref(store), _ptr(offsets), C.c_int64(total),
                       *[_ptr(flat.get(f)) for f in fields], *[_ptr(extra.get(f)) for f in ("env", "row", "tab0", "tabk", "tabA")],
                       self._stream())

    def q_update(self, k: int, s, action, r, cont, sn, W: torch.Tensor, apply: bool = True) -> None:
        n = s[0].numel()
        if n > self.n_envs:
            raise ScgError("q_update: more transitions than the context's n_envs")
        x, y, vx, vy = self._chk4(s, n, "s")
        xn, yn, vxn, vyn = self._chk4(sn, n, "s_next")
        self._chk(action, torch.uint8, n, "action"); self._chk(r, torch.float32, n, "r")
        self._chk(cont, torch.float32, n, "cont")
        _chk_W(self, W)
        if n and int(action.max()) >= NUM_ACTIONS:
            raise ScgError("action out of range [0, 5)")
        self._call("scg_q_update", n, k, _ptr(x), _ptr(y), _ptr(vx), _ptr(vy), _ptr(action), _ptr(r), _ptr(cont),
                   _ptr(xn), _ptr(yn), _ptr(vxn), _ptr(vyn), _ptr(W), C.c_uint32(STEP_APPLY if apply else 0),
                   self._stream())

    def classifier_predict(self, x: torch.Tensor, y: torch.Tensor, w8: torch.Tensor) -> torch.Tensor:
        n = x.numel()
        self._chk(x, torch.float32, n, "x"); self._chk(y, torch.float32, n, "y")
        self._chk(w8, torch.float32, CLF_STRIDE, "w8")
        out = torch.empty(n, dtype=torch.uint8, device=self.device)
        self._call("scg_classifier_predict", n, _ptr(x), _ptr(y), _ptr(w8), _ptr(out), self._stream())
        return out

    def classifier_logits(self, x: torch.Tensor, y: torch.Tensor, w8: torch.Tensor) -> torch.Tensor:
        """SPEC §24.2: the float32 value whose sign classifier_predict tests, by the same device function."""
        n = x.numel()
        self._chk(x, torch.float32, n, "x"); self._chk(y, torch.float32, n, "y")
        self._chk(w8, torch.float32, CLF_STRIDE, "w8")
        z = torch.empty(n, dtype=torch.float32, device=self.device)
        if n == 0:                                             # (an empty tensor has no address to pass)
            return z
        self._call("scg_classifier_logits", n, _ptr(x), _ptr(y), _ptr(w8), _ptr(z), self._stream())
        return z

    def fit_initiation(self, xy: torch.Tensor, label: torch.Tensor, offsets: torch.Tensor, w: torch.Tensor,
                       iters: int = 200, lr: float = 1.0, l2: float = 1e-4) -> None:
        n_fit = offsets.numel() - 1
        self._chk(offsets, torch.int32, n_fit + 1, "offsets")
        off = offsets.cpu()
        m = int(off[-1])
        if n_fit < 0 or int(off[0]) != 0 or bool((off[1:] < off[:-1]).any()):
            raise ScgError("offsets must start at 0 and be non-decreasing")
        self._chk(xy, torch.float32, 2 * m, "xy"); self._chk(label, torch.uint8, m, "label")
        self._chk(w, torch.float32, n_fit * CLF_STRIDE, "w")
        self._call("scg_fit_initiation", n_fit, _ptr(xy), _ptr(label), _ptr(offsets), _ptr(w), iters,
                   C.c_float(lr), C.c_float(l2), self._stream())
        # a fit whose workgroups could not run together gives up on the device (rows of w untouched) and says so in the
        # ctx's status word: the outer loop is about to act on these classifiers, so wait and look now (rare call)
        self.async_status(synchronize=True)

    # ------------------------------------------------------------------ asynchronous failures (include/scg_abi.h)
    def async_status(self, synchronize: bool = False) -> int:
        """Raise ScgError if a kernel launched earlier gave up on the device (sticky until clear_async_error);
        returns the raw status word otherwise (0)."""
        word = C.c_uint32(0)
        self._call("scg_async_status", self._stream(), 1 if synchronize else 0, C.byref(word))
        return int(word.value)

    def clear_async_error(self) -> None:
        self._call("scg_clear_async_error")

    def set_fit_timeout(self, seconds: float) -> None:
        """How long fit_initiation waits for a workgroup that is not running yet before it abandons that fit."""
        self._call("scg_set_fit_timeout", C.c_double(seconds))

    # ------------------------------------------------------------------ peer transport (include/scg_abi.h)
    def peer_export(self) -> bytes:
        """Allocate this rank's peer region (once) and return its 64-byte IPC handle."""
        buf = C.create_string_buffer(_lib.PEER_HANDLE_BYTES)
        self._call("scg_peer_export", C.cast(buf, C.c_void_p))
        return buf.raw

    def peer_open(self, n_ranks: int, rank: int, handles) -> None:
        """Map every rank's region: `handles` = the n_ranks 64-byte handles of peer_export, in rank order. From now on every
        learning step leaves its packed operand in this rank's region (step(..., apply=False))."""
        handles = [bytes(h) for h in handles]
        if len(handles) != n_ranks or any(len(h) != _lib.PEER_HANDLE_BYTES for h in handles):
            raise ScgError(f"peer_open: need {n_ranks} handles of {_lib.PEER_HANDLE_BYTES} bytes")
        blob = C.create_string_buffer(b"".join(handles), n_ranks * _lib.PEER_HANDLE_BYTES)
        self._call("scg_peer_open", C.c_int32(n_ranks), C.c_int32(rank), C.cast(blob, C.c_void_p))
        self.peer_ranks = int(n_ranks)

    def peer_exchange_apply(self, W: torch.Tensor) -> None:
        """After a learning step: publish this rank's operand, wait for every rank's, apply their rank-order sum to W
        (all on the device, on the current stream)."""
        _chk_W(self, W)
        self._call("scg_peer_exchange_apply", _ptr(W), self._stream())

    def set_peer_timeout(self, seconds: float) -> None:
        """How long the peer wait polls for a rank's epoch before it gives up (SCG_ASYNC_PEER_TIMEOUT, W untouched)."""
        self._call("scg_set_peer_timeout", C.c_double(seconds))

    @property
    def step_grid(self) -> int:
        """Workgroups of one fused step launch (one block of block_envs envs each)."""
        return -(-self.n_envs // self.block_envs)


class EnvState:
    """SoA env batch in HBM (caller-owned torch tensors)."""

    FIELDS = ("x", "y", "vx", "vy", "option_id", "opt_steps", "ep_steps", "qcache", "action", "reward", "done")

    def __init__(self, n: int, device: torch.device, pmap: PinballMap):
        z = lambda dt: torch.zeros(n, dtype=dt, device=device)
        sx, sy = float(pmap.starts[0][0]), float(pmap.starts[0][1])
        self.n = n
        self.x = torch.full((n,), sx, dtype=torch.float32, device=device)
        self.y = torch.full((n,), sy, dtype=torch.float32, device=device)
        self.vx, self.vy = z(torch.float32), z(torch.float32)
        self.option_id, self.opt_steps, self.ep_steps = z(torch.int32), z(torch.int32), z(torch.int32)
        self.qcache = torch.zeros((NUM_ACTIONS, n), dtype=torch.float32, device=device)
        self.action, self.done = z(torch.uint8), z(torch.uint8)
        self.reward = z(torch.float32)

    def state(self):
        return (self.x, self.y, self.vx, self.vy)
