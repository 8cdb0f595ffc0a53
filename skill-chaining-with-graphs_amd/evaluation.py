"""EpisodeStats — the per-env counters of an acting rollout (SPEC §8, scg_rollout; §11, scg_rollout_interrupt) and their
host-side summary."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._lib import RolloutStats


class EpisodeStats:
    """Counter tensors of SPEC §8 for `n` envs and `n_vf` value functions (root + options), zeroed. They are in/out:
    several rollout launches add up into one evaluation; `zero_()` starts a new one. `interrupts` ([n_vf][n], SPEC §11) is kept
    apart from FIELDS (the scg_rollout_stats members): an interrupting rollout counts into it and sets `interrupting`, which
    adds it to per_env() and summary(). `overrides` ([n_vf][n], SPEC §14) exists only once a value-ranking rollout asked for it
    (want_overrides()), and then shows in both as well."""

    FIELDS = ("ep_return", "ret_sum", "episodes", "goals", "len_sum", "vf_steps", "entries", "declines", "successes",
              "finished")

    def __init__(self, n_vf: int, n: int, device="cpu"):
        self.n_vf, self.n = int(n_vf), int(n)
        dev = torch.device(device)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        self.ep_return = z(n, torch.float32)
        self.ret_sum = z(n, torch.float64)
        self.episodes, self.goals, self.len_sum = z(n, torch.int32), z(n, torch.int32), z(n, torch.int32)
        self.vf_steps, self.entries = z((n_vf, n), torch.int32), z((n_vf, n), torch.int32)
        self.declines, self.successes = z((n_vf, n), torch.int32), z((n_vf, n), torch.int32)
        self.finished = z(n, torch.uint8)
        self.interrupts = z((n_vf, n), torch.int32)
        self.interrupting = False
        self.overrides = None          # [n_vf][n] int32 (SPEC §14), created by want_overrides(): a value-ranking rollout asks

    def want_overrides(self) -> torch.Tensor:
        """The `overrides` counters of a value-ranking rollout (SPEC §14), created zeroed on first use; from then on they show in
        per_env() and summary(), until zero_()."""
        if self.overrides is None:
            self.overrides = torch.zeros((self.n_vf, self.n), dtype=torch.int32, device=self.device)
        return self.overrides

    @property
    def device(self) -> torch.device:
        return self.episodes.device

    def zero_(self) -> "EpisodeStats":
        for f in self.FIELDS:
            getattr(self, f).zero_()
        self.interrupts.zero_()
        self.interrupting = False
        self.overrides = None
        return self

    def c_struct(self) -> RolloutStats:
        """The scg_rollout_stats of these tensors (device pointers; the tensors must stay alive while it is in use)."""
        return RolloutStats(**{f: C.c_void_p(getattr(self, f).data_ptr()) for f in self.FIELDS})

    def per_env(self) -> dict:
        out = {f: getattr(self, f) for f in self.FIELDS}
        if self.interrupting:
            out["interrupts"] = self.interrupts
        if self.overrides is not None:
            out["overrides"] = self.overrides
        return out

    def summary(self) -> dict:
        """Aggregate over the envs on the host in float64, in env order: episodes, success_rate, mean_return, mean_length
        (NaN with no episode recorded) and per value function k (index 0 = the root): steps_share (fraction of all steps
        run under k), entries, declines, successes; after an interrupting rollout also interrupts (SPEC §11), after a
        value-ranking one also overrides (SPEC §14: entries of an option that was not the lowest-numbered candidate)."""
        host = {f: getattr(self, f).detach().cpu().numpy() for f in self.FIELDS}
        eps = int(host["episodes"].astype(np.int64).sum())
        goals = int(host["goals"].astype(np.int64).sum())
        lens = int(host["len_sum"].astype(np.int64).sum())
        rets = host["ret_sum"].astype(np.float64)
        ret_total = float(np.cumsum(rets)[-1]) if rets.size else 0.0          # sequential, in env order
        steps = host["vf_steps"].astype(np.int64).sum(axis=1)
        all_steps = int(steps.sum())
        nan = float("nan")
        out = {
            "episodes": eps,
            "success_rate": goals / eps if eps else nan,
            "mean_return": ret_total / eps if eps else nan,
            "mean_length": lens / eps if eps else nan,
            "steps_share": [float(s) / all_steps if all_steps else nan for s in steps],
            "entries": [int(v) for v in host["entries"].astype(np.int64).sum(axis=1)],
            "declines": [int(v) for v in host["declines"].astype(np.int64).sum(axis=1)],
            "successes": [int(v) for v in host["successes"].astype(np.int64).sum(axis=1)],
        }
        if self.interrupting:
            out["interrupts"] = [int(v) for v in self.interrupts.detach().cpu().numpy().astype(np.int64).sum(axis=1)]
        if self.overrides is not None:
            out["overrides"] = [int(v) for v in self.overrides.detach().cpu().numpy().astype(np.int64).sum(axis=1)]
        return out
