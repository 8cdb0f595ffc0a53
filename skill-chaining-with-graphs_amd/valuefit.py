"""Least-squares value fits on recorded episodes. SPEC §16: the Monte-Carlo targets and the ridge solve of the normal equations
whose matrix scg_feature_gram forms. SPEC §17: the items of the least-squares TD fixed point (LSTD-Q) and the solve of its
block system, whose off-diagonal part scg_feature_cross_gram forms. SPEC §20: the targets of a fit to all-action branch returns, the
solve of one matrix against a right-hand side per action (scg_feature_gram_targets forms both) and the greedy-action table of its
report. SPEC §22: the precision weights of that fit, their normalisation and the root weights scg_feature_gram_weighted takes. Host
code, float64; the hot parts are ScgContext.feature_gram, feature_gram_targets, feature_gram_weighted and feature_cross_gram."""
from __future__ import annotations

import numpy as np
import torch

from ._lib import TRIAL_SUCCESS, ScgError
from .trajectory import DeviceRecord, Trajectory, _np_dtype


def returns_to_go(traj, gamma: float, r_option_success: float, device="cpu") -> dict:
    """SPEC §16.2 on a Trajectory of one-episode rollouts (or its to_numpy() dict): for every row, in (env, row) order as
    to_numpy() lays them out, float64
      g       the discounted task return-to-go  g_j = reward[j] + gamma g_{j+1},  g_L = 0  (a time limit is terminal)
      y       the target: g_j, plus gamma^(tau - j) r_option_success on a row of option o >= 1 whose execution ends, at row tau,
              in SUCCESS; tau is the first row >= j of the run of rows with vf = o whose term is not 0 (Trajectory.segments'
              cut), or the run's last row: a TIMEOUT followed at once by a new entry of the same option earns no bonus
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
    tau = torch.zeros(n, dtype=torch.int64, device=dev)            # the last row of the execution the row below belongs to ...
    succ = torch.zeros(n, dtype=torch.bool, device=dev)            # ... and whether that row's term is SUCCESS
    disc = torch.tensor([float(gamma) ** k * float(r_option_success) for k in range(rows + 1)], dtype=torch.float64, device=dev)
    for j in range(rows - 1, 0, -1):
        live = j < Lt
        g[:, j] = torch.where(live, reward[:, j] + gamma * g[:, j + 1], g[:, j])
        # an execution ends with the env's last row, before a row of another vf, and on a row whose option ended (term != 0):
        # an option that timed out and was entered again at once is two executions under one vf
        new_run = (j + 1 >= Lt) | (vf[:, j + 1] != vf[:, j]) | (term[:, j] != 0)
        tau = torch.where(new_run, torch.full_like(tau, j), tau)
        succ = torch.where(new_run, term[:, j] == TRIAL_SUCCESS, succ)
        bonus = torch.where(succ & (vf[:, j] >= 1), disc[tau - j], torch.zeros_like(g[:, j]))
        y[:, j] = torch.where(live, g[:, j] + bonus, y[:, j])
    e, r = torch.from_numpy(env).to(dev), torch.from_numpy(row).to(dev)
    return {"offsets": off, "g": g[e, r].cpu().numpy(), "y": y[e, r].cpu().numpy(), "sample": row >= 1}


def _checked_offsets(name: str, flat) -> np.ndarray:
    """The record's offsets as a contiguous int64 [n_env + 1], refused unless non-decreasing and inside [0, total]."""
    off = np.ascontiguousarray(np.asarray(flat["offsets"], np.int64).reshape(-1))
    if len(off) < 1 or off[0] < 0 or off[-1] > len(flat["reward"]) or np.any(np.diff(off) < 0):
        raise ScgError(f"{name}: offsets must be non-decreasing and inside [0, total]")
    return off


def row_tables(flat) -> dict:
    """The per-row tables of a flat record (to_numpy()'s dict), host arrays [total], the one host spelling of SPEC §28.2 / §30.1:
      env, row  int32: the env that owns the row and the row's index in it; -1 and 0 on a row no env owns (offsets[0] > 0,
                offsets[-1] < total)
      sample    bool: row >= 1, a step row (False on every env's row 0, the begin row, and on the rows no env owns)
      tab0      uint8: table 0 on the rows that are not done, else ROW_NONE
      tabk      uint8: the row's own table on the rows with vf >= 1 whose option goes on (term = 0, not done), else ROW_NONE
      tabA      uint8: the table that ACTS on the next row, vf[i + 1], where row i + 1 belongs to the same env and row i ended no
                episode (done = 0, or an env's row 0: a recorded begin row carries done = 2, SPEC §10), else ROW_NONE."""
    from ._lib import ROW_NONE
    off = np.asarray(flat["offsets"], np.int64).reshape(-1)
    done, vf, term = (np.asarray(flat[f], np.uint8) for f in ("done", "vf", "term"))
    total = len(done)
    L = np.diff(off)
    env, row, last = np.full(total, -1, np.int32), np.zeros(total, np.int32), np.ones(total, bool)
    if len(L):
        e = np.repeat(np.arange(len(L)), L)
        env[off[0]: off[-1]] = e
        row[off[0]: off[-1]] = np.arange(off[0], off[-1]) - off[:-1][e]
        last[off[0]: off[-1]] = row[off[0]: off[-1]] == L[e] - 1
    nxt = np.concatenate([vf[1:], np.zeros(min(total, 1), np.uint8)])                 # vf[i + 1] (unused on the last row)
    return {"env": env, "row": row, "sample": row >= 1,
            "tab0": np.where(done == 0, 0, ROW_NONE).astype(np.uint8),
            "tabk": np.where((vf >= 1) & (term == 0) & (done == 0), vf, ROW_NONE).astype(np.uint8),
            "tabA": np.where(~last & ((row == 0) | (done == 0)), nxt, ROW_NONE).astype(np.uint8)}


def flat_view(ctx, flat) -> dict:
    """A flat record (Trajectory.to_numpy()'s dict) as DeviceRecord.flat() gives one: `offsets` (int64 [n + 1]), one [total] tensor
    per recorded field in Trajectory's dtypes, `env`, `row`, `tab0`, `tabk`, `tabA` (row_tables') on ctx's device, and `total`
    (int). One upload per array, no library call; by bits DeviceRecord.from_trajectory(ctx, traj).flat()."""
    up = lambda v, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(v, dt))).to(ctx.device)
    tabs = row_tables(flat)
    out = {"offsets": up(np.reshape(flat["offsets"], -1), np.int64), "total": len(tabs["row"])}
    out.update({f: up(flat[f], _np_dtype(Trajectory.DTYPES[f])) for f in Trajectory.FIELDS if f in flat})
    out.update({f: up(tabs[f], tabs[f].dtype) for f in DeviceRecord.TABLES})
    return out


def sweep_targets(ctx, fl, W, gamma: float, lam, r_option_success: float, traced: bool = False, cut: bool = False, W_val=None) -> dict:
    """The targets of one sweep over a flat view `fl` (flat_view's or DeviceRecord.flat()'s) under the tables W, as device tensors
    [total]; the one values-then-scan sequence of SPEC §27.3 / §28.2 / §29.2. ScgContext.row_values gives `v0` (on tab0 under table
    0) and `vk` (on tabk); with a valuing table `W_val` ScgContext.row_values_cross gives them instead — W's greedy action valued
    under W_val — and `vs0`, `vsk`, W's own maxima. Not `traced` (`lam` a float): ScgContext.lambda_returns scans `y0`, `yk`.
    `traced` (`lam` a float or one per table): a third row_values call gives `ag` on tabA, ScgContext.trace_returns scans `y0`,
    `yk` and `h` with the trace cut at the off-greedy rows where `cut`, and formed here are `cut` (bool: the step rows whose recorded
    action is not ag of the row before, whether or not the trace is cut) and `c` (float64: the coefficient each step row carries,
    +0 on the other rows). `y` is yk on the rows with vf >= 1, y0 elsewhere."""
    from ._lib import NUM_ACTIONS, NUM_FEATURES
    Wt = W.contiguous().view(-1, NUM_ACTIONS, NUM_FEATURES)
    states = [fl[f] for f in ("x", "y", "vx", "vy")]
    out = {}
    if W_val is None:
        v0, _ = ctx.row_values(states, fl["tab0"], Wt[:1], actions=False)
        vk, _ = ctx.row_values(states, fl["tabk"], Wt, actions=False)
    else:
        Wv = W_val.contiguous().view(-1, NUM_ACTIONS, NUM_FEATURES)
        v0, _, out["vs0"] = ctx.row_values_cross(states, fl["tab0"], Wt[:1], Wv[:1], actions=False, sel_values=True)
        vk, _, out["vsk"] = ctx.row_values_cross(states, fl["tabk"], Wt, Wv, actions=False, sel_values=True)
    record = [fl[f] for f in ("offsets", "reward", "done", "vf", "term")]
    if traced:
        lam_vf = [float(lam)] * int(Wt.shape[0]) if np.ndim(lam) == 0 else [float(v) for v in lam]
        _, ag = ctx.row_values(states, fl["tabA"], Wt, actions=True)
        y0, yk, h = ctx.trace_returns(*record, fl["action"], ag, v0, vk, float(gamma), lam_vf, float(r_option_success), cut=bool(cut),
                                      horizon=True)
        step, vf = fl["row"] >= 1, fl["vf"].long()
        off_greedy = torch.zeros_like(step)
        off_greedy[1:] = step[1:] & (fl["action"][1:] != ag[:-1])
        c = torch.tensor(lam_vf, dtype=torch.float64, device=vf.device)[torch.where(vf < len(lam_vf), vf, torch.zeros_like(vf))]
        c = torch.where(step & ~off_greedy if cut else step, c, torch.zeros_like(c))
        out = {"ag": ag, "h": h, "c": c, "cut": off_greedy, **out}
    else:
        y0, yk = ctx.lambda_returns(*record, v0, vk, float(gamma), float(lam), float(r_option_success))
    return {"y0": y0, "yk": yk, "y": torch.where(fl["vf"] >= 1, yk, y0), "v0": v0, "vk": vk, **out}


def host_targets(fl, targets) -> dict:
    """sweep_targets' dict downloaded, with the view's `offsets` and `sample` (False on every env's row 0): what lambda_targets,
    trace_targets and double_targets return."""
    host = {f: v.cpu().numpy() for f, v in targets.items()}
    return {"offsets": fl["offsets"].cpu().numpy(), **{f: host.pop(f) for f in ("y0", "yk", "y")},
            "sample": (fl["row"] >= 1).cpu().numpy(), **host}


def trace_targets(ctx, flat, W, gamma: float, lam, r_option_success: float, cut: bool = True) -> dict:
    """SPEC §28.2: lambda_targets with a trace coefficient per row (ScgContext.trace_returns). `lam`: a float, or one float per value
    function. Beside lambda_targets' two row_values calls a third gives `ag`, the greedy action at every row's state of the table
    that ACTS on the next row — tabA[i] = vf[i + 1] where row i + 1 belongs to the same env and row i ended no episode (done = 0,
    or an env's row 0: a recorded begin row carries done = 2), else ROW_NONE (ag = 255) —; with `cut` the trace is cut to +0 on
    every row whose recorded action is not that action (Watkins's Q(lambda): the targets evaluate the greedy policy of W), without
    it `ag` is formed for the report only. Returns lambda_targets' dict plus `ag` (uint8), `h` (float64: the root stream's effective
    length, SPEC §28.1), `c` (float64: the coefficient each step row carries; +0 on an env's row 0) and
    `cut` (bool: the step rows whose recorded action is not the greedy one, whether or not `cut` is set)."""
    return _trace_targets("trace_targets", ctx, flat, W, None, gamma, lam, r_option_success, cut)


def double_targets(ctx, flat, W_sel, W_val, gamma: float, lam, r_option_success: float, cut: bool = False) -> dict:
    """SPEC §29.2: trace_targets with a double estimator in the bootstrap. `v0` and `vk` come from ScgContext.row_values_cross — the
    greedy action of W_sel at the row's state, valued under W_val (tab0, tabk as trace_targets forms them) — and `ag` is the greedy
    action under W_sel; the scan is ScgContext.trace_returns, untouched. Returns trace_targets' dict plus `vs0` and `vsk` (float32:
    W_sel's own maximum on the same rows, what a single estimator would bootstrap from). With W_val = W_sel every entry is
    trace_targets(W_sel)'s by bits and vs0 = v0, vsk = vk."""
    return _trace_targets("double_targets", ctx, flat, W_sel, W_val, gamma, lam, r_option_success, cut)


def _trace_targets(name: str, ctx, flat, W, W_val, gamma: float, lam, r_option_success: float, cut: bool) -> dict:
    """trace_targets (W_val None: the bootstrap values by row_values under W) and double_targets (by row_values_cross: W selects,
    W_val values), one copy."""
    from ._lib import NUM_ACTIONS, NUM_FEATURES
    flat = flat.to_numpy() if isinstance(flat, Trajectory) else flat
    _checked_offsets(name, flat)
    n_tab = W.numel() // (NUM_ACTIONS * NUM_FEATURES)
    lam_vf = [float(lam)] * n_tab if np.ndim(lam) == 0 else [float(v) for v in lam]
    if len(lam_vf) != n_tab or not all(0.0 <= v <= 1.0 for v in lam_vf) or not (0.0 <= float(gamma) <= 1.0):
        raise ScgError(f"{name}: gamma and lam (a float, or one per value function) must lie in [0, 1]")
    if W_val is not None and W_val.numel() != W.numel():
        raise ScgError(f"{name}: W_sel and W_val must have one shape")
    fl = flat_view(ctx, flat)
    return host_targets(fl, sweep_targets(ctx, fl, W, gamma, lam, r_option_success, traced=True, cut=cut, W_val=W_val))


def lambda_targets(ctx, flat, W, gamma: float, lam: float, r_option_success: float) -> dict:
    """SPEC §27.3: the lambda-return targets of a record (a Trajectory or its to_numpy() dict) under the value tables W
    [n_vf][5][1296] (a tensor on ctx's device), formed on the device: the flat record is uploaded, ScgContext.row_values gives
    every row's bootstrap values — v0 under table 0 on the rows that are not done, vk under the row's own table on the rows with
    vf >= 1 whose option goes on (term = 0, not done); +0 elsewhere, where §27.2 reads neither — and ScgContext.lambda_returns scans
    the two streams. Returns, in (env, row) order as returns_to_go does: `offsets`, `y0` and `yk` (float64), `y` (yk on the rows
    with vf >= 1, y0 elsewhere: consumable where returns_to_go()["y"] is), `sample` (False on every env's row 0) and `v0`, `vk`
    (float32). lam = 1 with every env ending done gives returns_to_go's g in y0 by bits; lam = 0 gives SPEC §17.2's targets.
    The offsets are checked here (non-decreasing, inside [0, total]) before anything is uploaded."""
    flat = flat.to_numpy() if isinstance(flat, Trajectory) else flat
    _checked_offsets("lambda_targets", flat)
    if not (0.0 <= float(lam) <= 1.0) or not (0.0 <= float(gamma) <= 1.0):
        raise ScgError("lambda_targets: gamma and lam must lie in [0, 1]")
    fl = flat_view(ctx, flat)
    return host_targets(fl, sweep_targets(ctx, fl, W, gamma, lam, r_option_success))


def fold_of(env) -> np.ndarray:
    """SPEC §29.2: the fold of each env of a record, int64: 0 (fold A) where env % 4 == 0, 1 (fold B) where env % 4 == 2 — together
    the even envs, the fit half of every fit here — and -1 on the odd envs, which stay held out."""
    env = np.asarray(env, np.int64)
    return np.where(env % 4 == 0, 0, np.where(env % 4 == 2, 1, -1)).astype(np.int64)


def mean_table(W_a, W_b):
    """SPEC §29.2: float32((float64 W_a + float64 W_b) / 2), the table a double fit hands on. Both must be float32 and of one shape
    (ValueError otherwise: a table of another type is not rounded to binary32 behind the caller's back). Tensors give a tensor on
    W_a's device, arrays an array."""
    as_np = lambda v: v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    a, b = as_np(W_a), as_np(W_b)
    if a.dtype != np.float32 or b.dtype != np.float32:
        raise ValueError(f"mean_table: the tables must be float32, not {a.dtype} and {b.dtype}")
    if a.shape != b.shape:
        raise ValueError(f"mean_table: W_a is {a.shape}, W_b {b.shape}")
    out = ((a.astype(np.float64) + b.astype(np.float64)) / 2.0).astype(np.float32)
    return torch.from_numpy(out).to(W_a.device) if isinstance(W_a, torch.Tensor) else out


def ridge_solve(A, b, n, ridge: float, scale, device=None) -> np.ndarray:
    """SPEC §16.3: Delta[a] = (A[a] + Lambda_a)^-1 b[a] with Lambda_a = diag(ridge max(n[a], 1) / scale_f^2), by a float64 Cholesky
    per action. A [n_act][F][F] symmetric (its lower triangle is read), b [n_act][F], n [n_act] sample counts, `scale` §3's
    table [F]. An action with n[a] = 0 gets Delta = 0 exactly. Returns float64 [n_act][F].
    With `device` a torch device the same system is factored there (A and b may be tensors on it): SPEC §18's fit at order 7 is
    five factorisations of 4096^2 per value function. The host path is the default and what §16's fit uses."""
    n = np.asarray(n, np.int64).reshape(-1)
    lam = 1.0 / np.asarray(scale, np.float64) ** 2
    if device is not None:
        At, bt = torch.as_tensor(A).to(device), torch.as_tensor(b).to(device)
        lam_t = torch.from_numpy(lam).to(device)
        out = np.zeros(tuple(bt.shape), np.float64)
        for a in range(At.shape[0]):
            if n[a] == 0:
                continue
            M = torch.tril(At[a].to(torch.float64))
            M = M + torch.tril(M, -1).T
            M.diagonal().add_(float(ridge) * max(int(n[a]), 1) * lam_t)
            Lc, info = torch.linalg.cholesky_ex(M)
            if int(info) != 0:
                raise ScgError(f"ridge_solve: the matrix of action {a} is not positive definite (leading minor {int(info)})")
            out[a] = torch.cholesky_solve(bt[a].to(torch.float64)[:, None], Lc)[:, 0].cpu().numpy()
        return out
    A, b = np.asarray(A, np.float64), np.asarray(b, np.float64)
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


def ridge_solve_shared(A, B, n, ridge: float, scale) -> np.ndarray:
    """SPEC §20.2: Delta[c] = (A + Lambda)^-1 B[c] for C right-hand sides B [C][F] of ONE matrix A [F][F] over n samples, Lambda =
    diag(ridge max(n, 1) / scale_f^2): one float64 Cholesky, then a solve per right-hand side with the calls ridge_solve makes, so
    that the result is by bits ridge_solve(repeat(A, C), B, [n] * C, ridge, scale). n = 0 gives zeros exactly. Returns float64 [C][F]."""
    B = np.asarray(B, np.float64)
    out = np.zeros_like(B)
    if int(n) == 0:
        return out
    lam = 1.0 / np.asarray(scale, np.float64) ** 2
    M = np.tril(np.asarray(A, np.float64))
    M = M + np.tril(M, -1).T
    M[np.diag_indices_from(M)] += float(ridge) * max(int(n), 1) * lam
    Lc = np.linalg.cholesky(M)
    for c in range(B.shape[0]):
        out[c] = np.linalg.solve(Lc.T, np.linalg.solve(Lc, B[c]))
    return out


def _pinned(name: str, ctx, A, B, n, ridge: float, scale, what: str):
    """ridge_solve_pinned and ridge_solve_shared_pinned, one copy: ScgContext.ridge_solve on A [n_mat][F][F] and B with lam = 1 /
    scale^2 and mu[g] = ridge max(n[g], 1) as ridge_solve forms them, the matrices with n[g] = 0 skipped; `info` is the one
    read-back, and a failed pivot raises ScgError naming the matrix (`what`) and the leading minor."""
    n = np.asarray(n, np.int64).reshape(-1)
    lam = torch.from_numpy(1.0 / np.asarray(scale, np.float64) ** 2).to(ctx.device)
    mu = [float(ridge) * max(int(v), 1) for v in n]
    delta, _, info = ctx.ridge_solve(A, B, lam, mu, skip=n == 0)
    info = info.cpu().numpy()
    if info.any():
        g = int(np.nonzero(info)[0][0])
        raise ScgError(f"{name}: the matrix{what.format(g)} is not positive definite (leading minor {int(info[g])})")
    return delta


def ridge_solve_pinned(ctx, A, b, n, ridge: float, scale) -> torch.Tensor:
    """SPEC §31.3: ridge_solve's system by ScgContext.ridge_solve — a float64 Cholesky on the device in SPEC §31.1's pinned order, the
    bits of which a host model reproduces, not LAPACK's. A float32 [n_act][F][F] and b float32 [n_act][F] are device tensors as the
    Gram calls return them and are not downloaded; n, ridge and `scale` as ridge_solve takes them; an action with n[a] = 0 gets
    Delta = 0 exactly; ScgError names the action and the leading minor of a matrix that is not positive definite. Returns Delta
    float64 [n_act][F] on the device."""
    return _pinned("ridge_solve_pinned", ctx, A, b, n, ridge, scale, " of action {}")


def ridge_solve_shared_pinned(ctx, A, B, n, ridge: float, scale) -> torch.Tensor:
    """SPEC §31.3: ridge_solve_shared's system by ScgContext.ridge_solve: ONE factorisation of A float32 [F][F] with the C rows of B
    float32 [C][F] as its right-hand sides (C <= 16), by bits ridge_solve_pinned(repeat(A, C), B, [n] * C, ridge, scale). n = 0
    gives zeros exactly. Returns Delta float64 [C][F] on the device."""
    F = int(A.shape[-1])
    return _pinned("ridge_solve_shared_pinned", ctx, A.view(1, F, F), B.view(1, -1, F), [int(n)], ridge, scale, "")[0]


def branch_targets(g, q_old):
    """SPEC §20.2: what a fit of Q to all-action branch returns regresses. g [M][A][R] (BranchResult.g: binary32), q_old [M][A]
    float32 (Q^old(s_i, a): the result's qcache). Returns
      gbar [M][A] float64   the mean of g over the replicates, summed in replicate order (BranchResult._moments)
      se2  [M][A] float64   s^2 / R with s^2 the unbiased variance: the squared standard error of gbar; 0 at R = 1
      D    [A][M] float32   float32(gbar - float64(q_old)) transposed: the residual, rounded once, a target per action as
                            ScgContext.feature_gram_targets takes them."""
    g = np.asarray(g, np.float32)
    q_old = np.asarray(q_old, np.float32)
    if g.ndim != 3 or g.shape[2] < 1 or q_old.shape != g.shape[:2]:
        raise ValueError("branch_targets: g must be [M][A][R] with R >= 1 and q_old [M][A]")
    R = g.shape[2]
    if R == 1:
        gbar, se2 = g[:, :, 0].astype(np.float64), np.zeros(g.shape[:2], np.float64)
    else:
        from .evaluation import BranchResult
        z = np.zeros(g.shape)
        gbar, var = BranchResult(np.zeros(g.shape[:2], np.uint8), g, z, z, z)._moments()
        se2 = var / R
    D = np.ascontiguousarray((gbar - q_old.astype(np.float64)).astype(np.float32).T)
    return gbar, se2, D


def normalise_weights(w) -> np.ndarray:
    """SPEC §22.2: w n / sum w, float64, the sum a plain chain in state order (per column of a [n][A] array): the weights of n
    samples with mean 1, so that §16.3's ridge term ridge max(n, 1) / scale^2 keeps its meaning. ValueError for an array that is
    not [n] or [n][A], for a negative or non-finite weight and for weights that sum to 0; weights that are all exactly 1 stay so."""
    w = np.array(w, np.float64)
    if w.ndim not in (1, 2) or not np.isfinite(w).all() or (w < 0).any():
        raise ValueError("weights must be a [n] or [n][A] array of finite values >= 0")
    if len(w) == 0:
        return w
    total = np.cumsum(w, axis=0)[-1]                           # (cumsum adds in index order; sum() adds pairwise)
    if np.any(total <= 0) or not np.isfinite(total).all():
        raise ValueError("weights must have a finite sum > 0")
    return w * len(w) / total


def precision_weights(se2, tau2=None, per_action: bool = False):
    """SPEC §22.2: the weights of a fit to branch means with the squared standard errors se2 [n][A] (branch_targets'): with
    v_i = mean_a se2[i][a] ([n]; per_action: v = se2 itself, a column of weights per action), w = 1 / (v + tau2), then
    normalise_weights. tau2 — the variance a target has beyond its replicates' spread; a parameter, not a constant of the method —
    defaults to the median of v, to the mean of v where that is 0, and where that is 0 too every weight is exactly 1. Returns
    (w float64, the tau2 used). ValueError for an se2 that is not [n][A], negative or non-finite, a tau2 that is negative or
    non-finite, and a tau2 of 0 given with some v of 0."""
    se2 = np.asarray(se2, np.float64)
    if se2.ndim != 2 or not np.isfinite(se2).all() or (se2 < 0).any():
        raise ValueError("se2 must be a [n][A] array of finite values >= 0")
    v = se2.copy() if per_action else (se2.mean(axis=1) if se2.shape[1] else np.zeros(len(se2)))
    if tau2 is None:
        tau2 = float(np.median(v)) if v.size else 0.0
        if tau2 == 0.0:
            tau2 = float(np.mean(v)) if v.size else 0.0
        if tau2 == 0.0:
            return np.ones(v.shape, np.float64), 0.0
    tau2 = float(tau2)
    if not np.isfinite(tau2) or tau2 < 0:
        raise ValueError("tau2 must be finite and >= 0")
    if tau2 == 0.0 and (v == 0).any():
        raise ValueError("tau2 = 0 with a target of variance 0: its weight would be infinite")
    return normalise_weights(1.0 / (v + tau2)), tau2


def root_weights(w) -> np.ndarray:
    """SPEC §22.2: what scg_feature_gram_weighted takes, float32(sqrt(float64 w)), rounded once. ValueError for a negative or
    non-finite weight."""
    w = np.asarray(w, np.float64)
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError("weights must be finite and >= 0")
    return np.sqrt(w).astype(np.float32)


def damped_tables(W, W_new, lambdas):
    """The candidates of a damped policy-improvement step (SPEC §21.4): row i is float32(float64(W) + lambdas[i] * (float64(W_new) -
    float64(W))), of W's shape behind the leading [len(lambdas)]; the rows of lambda = 0 and lambda = 1 are W and W_new themselves,
    by bits (the float64 difference is inexact where the two differ widely in magnitude). Tensors give a tensor on W's device,
    arrays an array."""
    as_np = lambda v: v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    w, wn = as_np(W).astype(np.float32), as_np(W_new).astype(np.float32)
    if w.shape != wn.shape:
        raise ValueError(f"damped_tables: W is {w.shape}, W_new {wn.shape}")
    lam = [float(v) for v in lambdas]
    d = wn.astype(np.float64) - w.astype(np.float64)
    out = np.stack([w if v == 0.0 else wn if v == 1.0 else (w.astype(np.float64) + v * d).astype(np.float32) for v in lam]) \
        if lam else np.zeros((0,) + w.shape, np.float32)
    return torch.from_numpy(out).to(W.device) if isinstance(W, torch.Tensor) else out


def choose_candidate(candidates, criterion: str = "discounted", z: float = 2.0) -> dict:
    """The decision rule of improve_policy (SPEC §21.4), a pure function: `candidates` is a list of {"lambda", "summary",
    "paired"} (paired: paired_differences against the current policy at the same epsilon). The candidate with the highest
    mean of `criterion` ("discounted": mean_discounted_return / paired disc_final; "return": mean_return / ret; "success":
    success_rate / goal) is picked, ties to the smallest lambda, a NaN mean never; it is accepted only where its paired
    mean_diff exceeds z * se (se = 0, fewer than two envs or every env the same difference: where it exceeds 0). Returns
    {"index" (the picked candidate's), "chosen_lambda" (0.0 when the current policy is kept), "accepted"}."""
    keys = {"discounted": ("mean_discounted_return", "disc_final"), "return": ("mean_return", "ret"), "success": ("success_rate", "goal")}
    if criterion not in keys:
        raise ValueError(f"criterion must be one of {sorted(keys)}, not {criterion!r}")
    mean_key, pair_key = keys[criterion]
    best = None
    for i, cand in enumerate(candidates):
        m, lam = float(cand["summary"][mean_key]), float(cand["lambda"])
        if m != m:
            continue
        if best is None or m > best[0] or (m == best[0] and lam < best[1]):
            best = (m, lam, i)
    if best is None:
        return {"index": None, "chosen_lambda": 0.0, "accepted": False}
    p = candidates[best[2]]["paired"][pair_key]
    accepted = bool(best[1] != 0.0 and p["mean_diff"] > (float(z) * p["se"] if p["se"] > 0.0 else 0.0))
    return {"index": best[2], "chosen_lambda": best[1] if accepted else 0.0, "accepted": accepted}


def greedy_table(gbar, q_old, q_new) -> dict:
    """SPEC §20.4: does acting greedily on Q^new pick better actions than on Q^old, judged by the branch means gbar [M][A]? With
    a_old, a_new, a* the FIRST maxima of q_old, q_new, gbar (each [M][A]):
      agreement_old, agreement_new   the share of states with a_old = a*, a_new = a*
      changed                        the share with a_new != a_old
      one_step_gain, one_step_gain_se   the mean over the states of gbar_i[a_new] - gbar_i[a_old] (exactly 0 where nothing changed)
                                     and its standard error (the unbiased standard deviation / sqrt(M); 0 with fewer than 2 states)
    Unbiased where gbar's replicates are not the ones q_new was fitted to (the held-out half). NaN without a state."""
    gbar = np.asarray(gbar, np.float64)
    M = gbar.shape[0]
    if M == 0:
        return {"n": 0, **{f: float("nan") for f in ("agreement_old", "agreement_new", "changed", "one_step_gain", "one_step_gain_se")}}
    idx = np.arange(M)
    a_old, a_new, a_star = (np.argmax(np.asarray(v), axis=1) for v in (q_old, q_new, gbar))
    gain = gbar[idx, a_new] - gbar[idx, a_old]
    se = float(np.sqrt(np.sum((gain - gain.mean()) ** 2) / (M - 1) / M)) if M >= 2 else 0.0
    return {"n": int(M), "agreement_old": float(np.mean(a_old == a_star)), "agreement_new": float(np.mean(a_new == a_star)),
            "changed": float(np.mean(a_new != a_old)), "one_step_gain": float(np.mean(gain)), "one_step_gain_se": se}


def error_stats(q, y) -> dict:
    """RMSE and mean error of predictions q against targets y (float64; NaN without samples)."""
    q, y = np.asarray(q, np.float64), np.asarray(y, np.float64)
    if len(y) == 0:
        return {"n": 0, "rmse": float("nan"), "mean_error": float("nan")}
    e = q - y
    return {"n": int(len(y)), "rmse": float(np.sqrt(np.mean(e * e))), "mean_error": float(np.mean(e))}


def fit_stats(q_old, q_new, y, y_mc, n_fit: int) -> dict:
    """The error block of a fit's report over one sample list, its first n_fit samples the fit half and the rest held out: "fit"
    and "held_out", each old / new error_stats of Q^old / Q^new against the targets y, and with y_mc (the Monte-Carlo targets of
    the same samples) "mc": the same two halves against those."""
    half = {"fit": slice(0, n_fit), "held_out": slice(n_fit, None)}
    block = lambda t: {name: {"old": error_stats(q_old[sl], t[sl]), "new": error_stats(q_new[sl], t[sl])} for name, sl in half.items()}
    return dict(block(y), mc=block(y_mc)) if y_mc is not None else block(y)


def trace_stats(targets, rows, ag_prev=None) -> dict:
    """What a traced fit reports of one target set (sweep_targets' dict) over the sample rows `rows` (a device index tensor), each
    NaN without a row: "cut_share" (the share whose incoming coefficient is 0), "off_greedy" (the share whose recorded action is
    not the greedy one), "horizon" (the mean effective length h of the root stream), the means in the order of `rows`, and
    "a_changed": the share whose greedy action differs from `ag_prev`'s (the sweep before's `ag`), None without one."""
    mean = lambda v: float(np.mean(v.cpu().numpy())) if len(rows) else float("nan")
    return {"cut_share": mean(targets["c"][rows] == 0.0), "off_greedy": mean(targets["cut"][rows]), "horizon": mean(targets["h"][rows]),
            "a_changed": None if ag_prev is None else mean(targets["ag"][rows - 1] != ag_prev[rows - 1])}


TD_CONT, TD_BOOT, TD_END = 0, 1, 2      # SPEC §17.2's kinds: bootstrap from Q_k(s'), from the root's value of s' (§5's exit rule), from nothing


def td_samples(traj, k: int, r_option_success: float = 0.0) -> dict:
    """SPEC §17.2's items of value function k on a Trajectory of one-episode rollouts (or its to_numpy() dict), in (env, row)
    order: `rows` (int64 indices into the flattened record: s' is that row's state, s the state of the row before), `env`,
    `kind` (uint8: TD_CONT / TD_BOOT / TD_END) and `r` (float64: the row's reward, plus r_option_success on an option's
    SUCCESS row). The root (k = 0) takes every step row of every env, kind CONT unless done (a time limit is terminal); option k
    the rows with vf = k, kind CONT while term = 0, BOOT where the option ends and the episode goes on, END where both end.
    There are no gestation items."""
    flat = traj.to_numpy() if isinstance(traj, Trajectory) else traj
    off = np.asarray(flat["offsets"], np.int64)
    L = np.diff(off)
    env = np.repeat(np.arange(len(L)), L)
    step = (np.arange(int(off[-1])) - off[:-1][env]) >= 1
    done, term = np.asarray(flat["done"]) != 0, np.asarray(flat["term"])
    if int(k) == 0:
        rows = np.nonzero(step)[0]
        kind = np.where(done[rows], TD_END, TD_CONT)
        r = np.asarray(flat["reward"], np.float64)[rows]
    else:
        rows = np.nonzero(step & (np.asarray(flat["vf"]) == int(k)))[0]
        kind = np.where(term[rows] == 0, TD_CONT, np.where(done[rows], TD_END, TD_BOOT))
        r = np.asarray(flat["reward"], np.float64)[rows] + np.where(term[rows] == TRIAL_SUCCESS, float(r_option_success), 0.0)
    return {"rows": rows.astype(np.int64), "env": env[rows], "kind": kind.astype(np.uint8), "r": r}


def greedy_max(q):
    """§5's max and its lowest index for q [5][n] (binary32 as scg_q_values gives it): m = q[0]; m = max(m, q[1]); ...;
    a' = the lowest a with q[a] = m. Returns (m float32 [n], a' int64 [n])."""
    q = np.asarray(q, np.float32)
    m = q[0].copy()
    for a in range(1, q.shape[0]):
        m = np.maximum(m, q[a])
    return m, np.argmax(q == m[None, :], axis=0).astype(np.int64)


def td_residual(r, kind, gamma: float, q_sa, m_k, m_0) -> np.ndarray:
    """SPEC §17.2: delta = r + gamma [CONT] m_k + gamma [BOOT] m_0 - Q_k(s, a), as (r + gamma m) - q in float64 (m the one
    maximum the sample's kind names, no term for END), rounded to binary32 once."""
    kind = np.asarray(kind)
    m = np.where(kind == TD_CONT, np.asarray(m_k, np.float64), np.where(kind == TD_BOOT, np.asarray(m_0, np.float64), 0.0))
    t = np.where(kind == TD_END, np.asarray(r, np.float64), np.asarray(r, np.float64) + float(gamma) * m)
    return (t - np.asarray(q_sa, np.float64)).astype(np.float32)


def lstdq_matrix(A, C, n, gamma: float, ridge: float, scale):
    """SPEC §17.3's matrix over the actions that have samples: (M float64 [m F][m F], act) with block (i, j) of M =
    [i = j] (A[a_i] + Lambda_{a_i}) - gamma C[a_i][a_j], a = act[.], Lambda_a = diag(ridge max(n[a], 1) / scale_f^2). A's lower
    triangle is read, as by ridge_solve."""
    A, C = np.asarray(A), np.asarray(C)
    n = np.asarray(n, np.int64).reshape(-1)
    F = A.shape[-1]
    act = [a for a in range(A.shape[0]) if n[a] > 0]
    lam = 1.0 / np.asarray(scale, np.float64) ** 2
    M = np.empty((len(act) * F, len(act) * F), np.float64)
    for i, a in enumerate(act):
        for j, a2 in enumerate(act):
            blk = M[i * F:(i + 1) * F, j * F:(j + 1) * F]
            blk[...] = C[a][a2]                             # (to float64 first: the product is not to be rounded to C's binary32)
            blk *= -float(gamma)
            if i == j:
                T = np.tril(A[a]).astype(np.float64)
                blk += T + np.tril(T, -1).T
                blk[np.diag_indices(F)] += float(ridge) * max(int(n[a]), 1) * lam
    return M, act


def lstdq_solve(A, C, b, n, gamma: float, ridge: float, scale, device=None) -> np.ndarray:
    """SPEC §17.3: Delta [n_act][F] float64 with M Delta = b, M as lstdq_matrix builds it from A [n_act][F][F], C
    [n_act][n_act][F][F], the counts n [n_act] and `scale` [F]; b [n_act][F]. A dense LU in float64, on the host (LAPACK) or, with
    `device` a torch device, there. Any F. An action with n[a] = 0 is taken out of the system and gets Delta = 0 exactly. A solve
    that fails or gives a non-finite value raises ScgError."""
    b = np.asarray(b, np.float64)
    M, act = lstdq_matrix(A, C, n, gamma, ridge, scale)
    out = np.zeros_like(b)
    if not act:
        return out
    rhs = np.concatenate([b[a] for a in act])
    try:
        if device is None:
            x = np.linalg.solve(M, rhs)
        else:
            x = torch.linalg.solve(torch.from_numpy(M).to(device), torch.from_numpy(rhs).to(device)).cpu().numpy()
    except (np.linalg.LinAlgError, RuntimeError) as e:
        raise ScgError(f"lstdq_solve: the {M.shape[0]} x {M.shape[0]} system could not be solved: {e}") from None
    if not np.isfinite(x).all():
        raise ScgError("lstdq_solve: the solution holds non-finite values")
    F = b.shape[1]
    for i, a in enumerate(act):
        out[a] = x[i * F:(i + 1) * F]
    return out


def lstdq_residual(A, C, b, n, gamma: float, ridge: float, scale, delta) -> float:
    """||M Delta - b|| / (||M|| ||Delta|| + ||b||) of a solution of SPEC §17.3's system (Frobenius / 2-norms, float64)."""
    M, act = lstdq_matrix(A, C, n, gamma, ridge, scale)
    if not act:
        return 0.0
    rhs = np.concatenate([np.asarray(b, np.float64)[a] for a in act])
    x = np.concatenate([np.asarray(delta, np.float64)[a] for a in act])
    den = np.linalg.norm(M) * np.linalg.norm(x) + np.linalg.norm(rhs)
    return float(np.linalg.norm(M @ x - rhs) / den) if den > 0 else 0.0
