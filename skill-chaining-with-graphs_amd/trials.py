"""TrialResult — the per-entry outputs of option trials (SPEC §9, scg_option_trials) and their host-side summary."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._lib import TRIAL_EPISODE_END, TRIAL_LEFT_INITIATION, TRIAL_SUCCESS, TRIAL_TIMEOUT, TrialOut

OUTCOMES = {TRIAL_SUCCESS: "success", TRIAL_EPISODE_END: "episode_end", TRIAL_LEFT_INITIATION: "left_initiation",
            TRIAL_TIMEOUT: "timeout"}


class TrialResult:
    """Output tensors of SPEC §9 for `n` trials, plus the option id each entry ran (`option`, int32 [n]). `outcome` is 0 for an
    entry that was not run; the other outputs of such an entry are left as allocated (zero)."""

    FIELDS = ("outcome", "steps", "ret", "disc_ret", "v0", "end_x", "end_y", "end_vx", "end_vy")

    def __init__(self, n: int, option=None, device="cpu"):
        self.n = int(n)
        dev = torch.device(device)
        z = lambda dt: torch.zeros(self.n, dtype=dt, device=dev)
        self.outcome, self.steps = z(torch.uint8), z(torch.int32)
        for f in self.FIELDS[2:]:
            setattr(self, f, z(torch.float32))
        self.option = z(torch.int32) if option is None else torch.as_tensor(option, dtype=torch.int32).to(dev).contiguous()

    @property
    def device(self) -> torch.device:
        return self.outcome.device

    def c_struct(self) -> TrialOut:
        """The scg_trial_out of these tensors (device pointers; the tensors must stay alive while it is in use)."""
        return TrialOut(**{f: C.c_void_p(getattr(self, f).data_ptr()) for f in self.FIELDS})

    def per_entry(self) -> dict:
        return {f: getattr(self, f) for f in self.FIELDS + ("option",)}

    def summary(self) -> dict:
        """Per option k that was run at least once: {k: {trials, rate of each outcome (success, episode_end, left_initiation,
        timeout), mean_steps_success (NaN without a success), mean_disc_ret, mean_v0}}. Computed on the host in float64, sums
        taken sequentially in entry order."""
        host = {f: getattr(self, f).detach().cpu().numpy() for f in self.FIELDS + ("option",)}
        oc, opt = host["outcome"].astype(np.int64), host["option"].astype(np.int64)
        out = {}
        for k in sorted(set(opt[oc != 0].tolist())):
            sel = (opt == k) & (oc != 0)
            n = int(sel.sum())
            succ = sel & (oc == TRIAL_SUCCESS)
            ns = int(succ.sum())

            def seq_sum(a):
                return float(np.cumsum(a.astype(np.float64))[-1]) if a.size else 0.0
            r = {"trials": n}
            for code, name in OUTCOMES.items():
                r[name] = int((sel & (oc == code)).sum()) / n
            r["mean_steps_success"] = seq_sum(host["steps"][succ]) / ns if ns else float("nan")
            r["mean_disc_ret"] = seq_sum(host["disc_ret"][sel]) / n
            r["mean_v0"] = seq_sum(host["v0"][sel]) / n
            out[int(k)] = r
        return out
