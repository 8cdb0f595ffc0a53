"""Least-squares value fit on realised returns (SPEC §16): the Monte-Carlo targets of recorded episodes and the ridge solve of
the normal equations whose matrix scg_feature_gram forms. Host code, float64; the hot part is ScgContext.feature_gram."""
from __future__ import annotations

import numpy as np
import torch

from ._lib import TRIAL_SUCCESS
from .trajectory import Trajectory


def returns_to_go(traj, gamma: float, r_option_success: float, device="cpu") -> dict:
    """SPEC §16.2 on a Trajectory of one-episode rollouts (or its to_numpy() dict): for every row, in (env, row) order as
    to_numpy() lays them out, float64
      g       the discounted task return-to-go  g_j = reward[j] + gamma g_{j+1},  g_L = 0  (a time limit is terminal)
      y       the target: g_j, plus gamma^(tau - j) r_option_success on a row of option o >= 1 whose run of rows with vf = o ends,
              at row tau, in SUCCESS
      sample  False on every env's row 0 (the begin row: no step), True elsewhere
    and `offsets` [n + 1]. Vectorised over the envs, a loop over the rows, on `device` (torch, float64)."""
    flat = traj.to_numpy() if isinstance(traj, Trajectory) else traj
    off = np.asarray(flat["offsets"], np.int64)
    n, total = len(off) - 1, int(off[-1])
    L = np.diff(off)
    rows = int(L.max()) if n else 0
    dev = torch.device(device)
    env = np.repeat(np.arange(n), L)
    row = np.arange(total) - off[:-1][env]
    pad = lambda v, dt: torch.zeros((n, rows + 1), dtype=dt).index_put_(
        (torch.from_numpy(env), torch.from_numpy(row)), torch.as_tensor(np.asarray(v)).to(dt)).to(dev)
    reward, vf, term = pad(flat["reward"], torch.float64), pad(flat["vf"], torch.int64), pad(flat["term"], torch.int64)
    Lt = torch.from_numpy(L).to(dev)
    g = torch.zeros((n, rows + 1), dtype=torch.float64, device=dev)
    y = torch.zeros_like(g)
    tau = torch.zeros(n, dtype=torch.int64, device=dev)            # the last row of the run the row below belongs to ...
    succ = torch.zeros(n, dtype=torch.bool, device=dev)            # ... and whether that row's term is SUCCESS
    for j in range(rows - 1, 0, -1):
        live = j < Lt
        g[:, j] = torch.where(live, reward[:, j] + gamma * g[:, j + 1], g[:, j])
        new_run = (j + 1 >= Lt) | (vf[:, j + 1] != vf[:, j])
        tau = torch.where(new_run, torch.full_like(tau, j), tau)
        succ = torch.where(new_run, term[:, j] == TRIAL_SUCCESS, succ)
        bonus = torch.where(succ & (vf[:, j] >= 1), float(r_option_success) * torch.pow(
            torch.full((n,), float(gamma), dtype=torch.float64, device=dev), (tau - j).to(torch.float64)), torch.zeros_like(g[:, j]))
        y[:, j] = torch.where(live, g[:, j] + bonus, y[:, j])
    e, r = torch.from_numpy(env).to(dev), torch.from_numpy(row).to(dev)
    return {"offsets": off, "g": g[e, r].cpu().numpy(), "y": y[e, r].cpu().numpy(), "sample": row >= 1}


def ridge_solve(A, b, n, ridge: float, scale) -> np.ndarray:
    """SPEC §16.3: Delta[a] = (A[a] + Lambda_a)^-1 b[a] with Lambda_a = diag(ridge max(n[a], 1) / scale_f^2), by a float64 Cholesky
    per action. A [n_act][F][F] symmetric (its lower triangle is read), b [n_act][F], n [n_act] sample counts, `scale` §3's
    table [F]. An action with n[a] = 0 gets Delta = 0 exactly. Returns float64 [n_act][F]."""
    A, b = np.asarray(A, np.float64), np.asarray(b, np.float64)
    n = np.asarray(n, np.int64).reshape(-1)
    lam = 1.0 / np.asarray(scale, np.float64) ** 2
    out = np.zeros_like(b)
    for a in range(A.shape[0]):
        if n[a] == 0:
            continue
        M = np.tril(A[a])
        M = M + np.tril(M, -1).T
        M[np.diag_indices_from(M)] += float(ridge) * max(int(n[a]), 1) * lam
        Lc = np.linalg.cholesky(M)
        out[a] = np.linalg.solve(Lc.T, np.linalg.solve(Lc, b[a]))
    return out


def error_stats(q, y) -> dict:
    """RMSE and mean error of predictions q against targets y (float64; NaN without samples)."""
    q, y = np.asarray(q, np.float64), np.asarray(y, np.float64)
    if len(y) == 0:
        return {"n": 0, "rmse": float("nan"), "mean_error": float("nan")}
    e = q - y
    return {"n": int(len(y)), "rmse": float(np.sqrt(np.mean(e * e))), "mean_error": float(np.mean(e))}

