"""EpisodeStats — the per-env counters of an acting rollout (SPEC §8, scg_rollout; §11, scg_rollout_interrupt) and their
host-side summary; GateAudit — the per-env arrays of an audited rollout (SPEC §15, scg_rollout_audit) and the summary of an
enter / decline pair of them; BranchResult — the returns of branch rollouts (SPEC §19, scg_rollout_branch) and their statistics;
paired_differences — the per-env differences of two policies evaluated on common random numbers (SPEC §21)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._lib import Audit, RolloutStats


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
        self.audit = None              # the GateAudit of an audited evaluation (SPEC §15): its disc_final shows in per_env()

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
        self.audit = None
        return self

    def c_struct(self) -> RolloutStats:
        """The scg_rollout_stats of these tensors (device pointers; the tensors must stay alive while it is in use)."""
        return RolloutStats(**{f: C.c_void_p(getattr(self, f).data_ptr()) for f in self.FIELDS})

    def _range(self, lo, hi):
        """The env range lo .. hi - 1 as a slice of the last axis (None, None: every env)."""
        lo, hi = 0 if lo is None else int(lo), self.n if hi is None else int(hi)
        if not (0 <= lo <= hi <= self.n):
            raise ValueError(f"env range {lo}..{hi} outside the {self.n} envs")
        return slice(lo, hi)

    def per_env(self, lo=None, hi=None) -> dict:
        """The per-env counter tensors; with `lo`, `hi` those of the envs lo .. hi - 1 (SPEC §21: one policy's range)."""
        out = {f: getattr(self, f) for f in self.FIELDS}
        if self.interrupting:
            out["interrupts"] = self.interrupts
        if self.overrides is not None:
            out["overrides"] = self.overrides
        if self.audit is not None:
            out["disc_final"] = self.audit.disc_final
        if lo is None and hi is None:
            return out
        r = self._range(lo, hi)
        return {f: v[..., r] for f, v in out.items()}

    def summary(self, lo=None, hi=None) -> dict:
        """Aggregate over the envs on the host in float64, in env order: episodes, success_rate, mean_return, mean_length
        (NaN with no episode recorded) and per value function k (index 0 = the root): steps_share (fraction of all steps
        run under k), entries, declines, successes; after an interrupting rollout also interrupts (SPEC §11), after a
        value-ranking one also overrides (SPEC §14: entries of an option that was not the lowest-numbered candidate).
        With `lo`, `hi`: over the envs lo .. hi - 1 only (SPEC §21: one policy's range of a population rollout)."""
        r = self._range(lo, hi)
        host = {f: getattr(self, f).detach().cpu().numpy()[..., r] for f in self.FIELDS}
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
            out["interrupts"] = [int(v) for v in self.interrupts.detach().cpu().numpy()[..., r].astype(np.int64).sum(axis=1)]
        if self.overrides is not None:
            out["overrides"] = [int(v) for v in self.overrides.detach().cpu().numpy()[..., r].astype(np.int64).sum(axis=1)]
        if self.audit is not None:
            d = self.audit.disc_final.detach().cpu().numpy()[r].astype(np.float64)[host["episodes"] > 0]
            out["mean_discounted_return"] = float(np.cumsum(d)[-1]) / d.size if d.size else nan
        return out


def _mean(v) -> float:
    """The float64 mean of `v` summed in order (NaN for none)."""
    v = np.asarray(v, np.float64)
    return float(np.cumsum(v)[-1]) / v.size if v.size else float("nan")


PAIRED_FIELDS = {"ret": "ret_sum", "disc_final": "disc_final", "goal": "goals", "steps": "len_sum"}


def paired_differences(per_env_a, per_env_b) -> dict:
    """Policy a against policy b on common random numbers (SPEC §21): `per_env_*` are two EpisodeStats.per_env() dicts of one
    length (tensors or arrays) of one-episode evaluations with the discounted return kept. For ret (ret_sum), disc_final, goal
    (goals) and steps (len_sum) returns {"mean_diff", "se", "n"} of the per-env differences a - b: host float64, summed in env
    order; se is their unbiased standard deviation / sqrt(n), 0 below two envs. Equal inputs give exact zeros."""
    out = {}
    for name, f in PAIRED_FIELDS.items():
        if f not in per_env_a or f not in per_env_b:
            raise ValueError(f"paired_differences: both per-env dicts need {f!r} (evaluate(discounted=True, per_env=True))")
        a, b = (np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v).astype(np.float64).reshape(-1)
                for v in (per_env_a[f], per_env_b[f]))
        if a.shape != b.shape:
            raise ValueError(f"paired_differences: {f} holds {a.size} and {b.size} envs")
        d, n = a - b, a.size
        mean = float(np.cumsum(d)[-1]) / n if n else float("nan")
        se = float(np.sqrt(np.cumsum((d - mean) ** 2)[-1] / (n - 1) / n)) if n >= 2 else 0.0
        out[name] = {"mean_diff": mean, "se": se, "n": int(n)}
    return out


class GateAudit:
    """The per-env arrays of an audited rollout (SPEC §15) for `n` envs: `force` (int8; +k: enter option k at the begin
    pseudo-step, -k: decline it, 0: the gate's own choice; None: not given), and the outputs applied (uint8), cand (int8), v_root,
    v_cand, disc_ret, disc_g, disc_final (float32; v_cand and disc_final start as NaN: written only where a candidate was offered /
    an episode ended). disc_ret and disc_g are in/out across the launches of one evaluation."""

    DTYPES = {"force": torch.int8, "applied": torch.uint8, "cand": torch.int8, "v_root": torch.float32, "v_cand": torch.float32,
              "disc_ret": torch.float32, "disc_g": torch.float32, "disc_final": torch.float32}

    def __init__(self, n: int, device="cpu", force=None):
        self.n = int(n)
        dev = torch.device(device)
        self.force = None if force is None else torch.as_tensor(force, dtype=torch.int8).to(dev).contiguous().view(-1)
        if self.force is not None and self.force.numel() != self.n:
            raise ValueError(f"force has {self.force.numel()} entries for {self.n} envs")
        self.applied = torch.zeros(self.n, dtype=torch.uint8, device=dev)
        self.cand = torch.zeros(self.n, dtype=torch.int8, device=dev)
        self.v_root = torch.zeros(self.n, dtype=torch.float32, device=dev)
        self.v_cand = torch.full((self.n,), float("nan"), dtype=torch.float32, device=dev)
        self.disc_ret = torch.zeros(self.n, dtype=torch.float32, device=dev)
        self.disc_g = torch.ones(self.n, dtype=torch.float32, device=dev)
        self.disc_final = torch.full((self.n,), float("nan"), dtype=torch.float32, device=dev)

    @property
    def device(self) -> torch.device:
        return self.applied.device

    def c_struct(self) -> Audit:
        """The scg_audit of these tensors (device pointers; the tensors must stay alive while it is in use)."""
        return Audit(**{f: None if getattr(self, f) is None else C.c_void_p(getattr(self, f).data_ptr()) for f in self.DTYPES})

    def host(self) -> dict:
        return {f: getattr(self, f).detach().cpu().numpy() for f in self.DTYPES if getattr(self, f) is not None}

    @staticmethod
    def pair_summary(option, v_k, v_0, g_enter, g_decline, goal_enter, goal_decline) -> dict:
        """The gate against the two branches it chooses between, over the audited states (host arrays of one length, in state
        order; float64 arithmetic): `option` the option offered, v_k / v_0 the values the gate compared, g_enter / g_decline the
        realised discounted task returns of the episode that entered / declined, goal_* whether that episode reached the goal.
        Returns {"overall": row, "options": {k: row}}; a row holds n, enter_rate (V_k >= V_0; a NaN declines), mean_v_k,
        mean_v_0, mean_g_enter, mean_g_decline, mean_advantage (G_enter - G_decline), agreement (the share of states where the
        gate's decision equals G_enter >= G_decline), regret (mean of max(G_enter, G_decline) - G of the branch the gate chose),
        calib_enter (mean V_k - G_enter), calib_decline (mean V_0 - G_decline), goal_rate_enter and goal_rate_decline. Means
        of no state are NaN."""
        option = np.asarray(option, np.int64)
        v_k, v_0, ge, gd = (np.asarray(v, np.float64) for v in (v_k, v_0, g_enter, g_decline))
        goal_e, goal_d = np.asarray(goal_enter, np.float64), np.asarray(goal_decline, np.float64)
        with np.errstate(invalid="ignore"):
            gate = v_k >= v_0
            better = ge >= gd
        chosen = np.where(gate, ge, gd)

        def row(m):
            return {
                "n": int(m.sum()),
                "enter_rate": _mean(gate[m]), "mean_v_k": _mean(v_k[m]), "mean_v_0": _mean(v_0[m]),
                "mean_g_enter": _mean(ge[m]), "mean_g_decline": _mean(gd[m]), "mean_advantage": _mean((ge - gd)[m]),
                "agreement": _mean((gate == better)[m]), "regret": _mean((np.maximum(ge, gd) - chosen)[m]),
                "calib_enter": _mean((v_k - ge)[m]), "calib_decline": _mean((v_0 - gd)[m]),
                "goal_rate_enter": _mean(goal_e[m]), "goal_rate_decline": _mean(goal_d[m]),
            }
        return {"overall": row(np.ones(option.shape, bool)),
                "options": {int(k): row(option == k) for k in sorted(set(option.tolist()))}}


class BranchResult:
    """The returns of branch rollouts (SPEC §19): M source states, A first actions per state, R replicates of each, every
    replicate resumed from the source's whole env state with that first action forced and continued under the current policy on
    a random stream of its own. Host arrays:
      actions [M][A] uint8   the forced first action of column a
      g       [M][A][R]      the discounted TASK return from the branch step on (SPEC §15's d of the episode's end, binary32)
      ret     [M][A][R]      the undiscounted return from the branch step on;  goal [M][A][R] bool;  steps [M][A][R] steps taken
    The statistics are host float64, in state order. They condition on the WHOLE env state (position, velocity, ep_steps,
    opt_steps, a declined id), not on (x, y, vx, vy) alone: spread() is the floor under a function of the whole state."""

    def __init__(self, actions, g, ret, goal, steps):
        self.actions = np.asarray(actions, np.uint8)
        self.g, self.ret = np.asarray(g, np.float32), np.asarray(ret, np.float64)
        self.goal, self.steps = np.asarray(goal, bool), np.asarray(steps, np.int64)
        if self.actions.ndim != 2 or self.g.ndim != 3 or self.g.shape[:2] != self.actions.shape:
            raise ValueError("BranchResult: actions must be [M][A] and g [M][A][R]")
        self.M, self.A, self.R = (int(v) for v in self.g.shape)

    def _moments(self):
        """(mean [M][A], unbiased variance [M][A]) of g over the replicates, float64, summed in replicate order."""
        if self.R < 2:
            raise ValueError("BranchResult: the within-state variance needs at least 2 replicates")
        g = self.g.astype(np.float64)
        mean = np.cumsum(g, axis=2)[:, :, -1] / self.R
        var = np.cumsum((g - mean[:, :, None]) ** 2, axis=2)[:, :, -1] / (self.R - 1)
        return mean, var

    def spread(self, g_recorded=None, column=0) -> dict:
        """The within-state spread of the return-to-go under action column `column` (the recorded action's; one for all states, or
        one per state [M]): n, spread_rmse =
        sqrt(mean_i s_i^2) with s_i^2 the unbiased variance over the R replicates (the noise floor under ANY function of the
        whole env state, whatever its basis), zero_variance (the share of states with s_i^2 = 0) and, with `g_recorded` [M] (the
        record's own return-to-go of each state), recorded_z2: the mean over the states with s_i^2 > 0 of (g_recorded - mean_i)^2
        / (s_i^2 (1 + 1/R)), near 1 where the record's continuation is one more draw from the replicates' distribution (NaN
        without such a state), and recorded_z2_median, the median of the same ratios. With s_i^2 estimated from R replicates the
        ratio is heavy-tailed: for normal returns it is F(1, R - 1), whose mean is (R - 1) / (R - 3) (1.4 at R = 8) and whose
        median is near 0.5, and a state whose replicates almost agree while the record took an exploring step can carry the
        whole mean. Read the median beside the mean."""
        mean, var = self._moments()
        col = np.broadcast_to(np.asarray(column, np.int64), (self.M,))
        mean, var = mean[np.arange(self.M), col], var[np.arange(self.M), col]
        out = {"n": self.M, "spread_rmse": float(np.sqrt(_mean(var))) if self.M else float("nan"),
               "zero_variance": _mean(var == 0)}
        if g_recorded is not None:
            gr = np.asarray(g_recorded, np.float64).reshape(-1)
            if gr.shape != (self.M,):
                raise ValueError(f"g_recorded must hold {self.M} entries")
            pos = var > 0
            z2 = (gr[pos] - mean[pos]) ** 2 / (var[pos] * (1.0 + 1.0 / self.R))
            out["recorded_z2"] = _mean(z2)
            out["recorded_z2_median"] = float(np.median(z2)) if z2.size else float("nan")
        return out

    def action_table(self, a_w) -> dict:
        """Is the action a value function prefers the best one? `a_w` [M]: the action to judge per state (the first maximum of
        the source's qcache), which must be one of the state's columns. With mean_i[a] the replicate mean of column a:
          greedy_agreement  mean(a_w == the action of argmax_a mean_i[a])  (first maximum)
          gap               mean(max_a mean_i[a] - mean_i[a_w]): BIASED UPWARDS by the noise, since the maximum of noisy means
                            exceeds the mean of the best action; it is >= 0 by construction even where every action is equal
          gap_holdout       the best action chosen on the even-indexed replicates, its mean minus a_w's evaluated on the
                            odd-indexed ones: the unbiased one-step improvement available (R must be even and >= 2)
          significant       the share of states whose gap_i exceeds twice its standard error sqrt((s_i^2[best] + s_i^2[a_w]) / R)
        and per_state: a_w, best (action ids), mean [M][A], var [M][A], gap, gap_holdout."""
        if self.R < 2 or self.R % 2:
            raise ValueError(f"BranchResult.action_table: replicates must be even and >= 2, not {self.R}")
        a_w = np.asarray(a_w, np.int64).reshape(-1)
        if a_w.shape != (self.M,):
            raise ValueError(f"a_w must hold {self.M} entries")
        hit = self.actions.astype(np.int64) == a_w[:, None]
        if not hit.any(axis=1).all():
            raise ValueError("a_w names an action that is not among a state's columns")
        cw, idx = np.argmax(hit, axis=1), np.arange(self.M)
        mean, var = self._moments()
        best = np.argmax(mean, axis=1)
        gap = mean[idx, best] - mean[idx, cw]
        g = self.g.astype(np.float64)
        half = self.R // 2
        even = np.cumsum(g[:, :, 0::2], axis=2)[:, :, -1] / half
        odd = np.cumsum(g[:, :, 1::2], axis=2)[:, :, -1] / half
        pick = np.argmax(even, axis=1)
        gap_h = odd[idx, pick] - odd[idx, cw]
        se = np.sqrt((var[idx, best] + var[idx, cw]) / self.R)
        return {"n": self.M, "greedy_agreement": _mean(best == cw), "gap": _mean(gap), "gap_holdout": _mean(gap_h),
                "significant": _mean(gap > 2.0 * se),
                "per_state": {"a_w": a_w, "best": self.actions[idx, best].astype(np.int64), "mean": mean, "var": var, "gap": gap,
                              "gap_holdout": gap_h}}
