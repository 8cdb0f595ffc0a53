"""Gate tables (SPEC §25): what the value gate of a population rollout compares, apart from the weights that act.

A gate table is float32 [n_vf][2][5][1296]: for option k >= 1, [k][0] is the OPTION side and [k][1] the ROOT side of k's gate,
`declined = entering && !(max_a Q(s_next, a | [k][0]) >= max_a Q(s_next, a | [k][1]))`; row 0 is never read. Everything here is
a pure function: no input is written, every table returned is a new tensor."""
from __future__ import annotations

import numpy as np
import torch

from ._lib import NUM_ACTIONS, NUM_FEATURES


def _weights(W) -> torch.Tensor:
    W = torch.as_tensor(W, dtype=torch.float32)
    if W.numel() % (NUM_ACTIONS * NUM_FEATURES) or W.numel() == 0:
        raise ValueError(f"W must be [n_vf, {NUM_ACTIONS}, {NUM_FEATURES}]")
    return W.reshape(-1, NUM_ACTIONS, NUM_FEATURES)


def _table(gate) -> torch.Tensor:
    gate = torch.as_tensor(gate, dtype=torch.float32)
    if gate.dim() != 4 or tuple(gate.shape[1:]) != (2, NUM_ACTIONS, NUM_FEATURES):
        raise ValueError(f"a gate table must be [n_vf, 2, {NUM_ACTIONS}, {NUM_FEATURES}], not {tuple(gate.shape)}")
    return gate


def shipped_gate(W) -> torch.Tensor:
    """The comparison SPEC §4.2 ships, as a table: [k][0] = W[k], [k][1] = W[0] for k >= 1, row 0 zeros. A population rollout with
    it equals the rollout without a gate table by bits (SPEC §25.1's identity)."""
    W = _weights(W)
    g = torch.zeros((W.shape[0], 2, NUM_ACTIONS, NUM_FEATURES), dtype=torch.float32, device=W.device)
    g[1:, 0] = W[1:]
    g[1:, 1] = W[0]
    return g


def always_enter(n_vf: int, device=None) -> torch.Tensor:
    """All zeros: both sides are 0 at every state, and 0 >= 0 enters."""
    return torch.zeros((int(n_vf), 2, NUM_ACTIONS, NUM_FEATURES), dtype=torch.float32, device=device)


def never_enter(n_vf: int, device=None) -> torch.Tensor:
    """[k][0][a][0] = -1 for every k and a, the rest 0: feature 0 has the all-zero coefficient vector and is exactly 1 (SPEC §3), so
    the option side is -1 at every state, the root side 0, and the gate declines."""
    g = always_enter(n_vf, device)
    g[:, 0, :, 0] = -1.0
    return g


def advantage_gate(base, u: dict) -> torch.Tensor:
    """`base` with the rows of the fitted options replaced: for each k of `u` ({k: u_k [1296]}), [k][0][a] = float32(u_k) for all
    five a and [k][1] = 0, so that the gate enters where u_k . phi(s_next) >= 0. Every other row is base's."""
    g = _table(base).clone()
    for k, uk in u.items():
        k = int(k)
        if not (1 <= k < g.shape[0]):
            raise ValueError(f"advantage_gate: option {k} is outside the table's rows 1 .. {g.shape[0] - 1}")
        row = torch.from_numpy(np.asarray(uk, np.float64).reshape(NUM_FEATURES).astype(np.float32)).to(g.device)
        g[k, 0] = row                                  # (broadcast over the five actions)
        g[k, 1] = 0.0
    return g


def candidate_gates(W, u: dict) -> list:
    """The candidate gate tables of improve_gate, initfit.candidate_tables' mirror: [(label, table)] with "shipped"
    (shipped_gate(W)), "always", "never", then "k" for each fitted k of `u`, ascending (row k alone replaced in the shipped gate),
    then "all" (every fitted row replaced) when two or more were fitted."""
    base = shipped_gate(W)
    n_vf, dev = base.shape[0], base.device
    ks = sorted(int(k) for k in u)
    out = [("shipped", base), ("always", always_enter(n_vf, dev)), ("never", never_enter(n_vf, dev))]
    out += [(str(k), advantage_gate(base, {k: u[k]})) for k in ks]
    if len(ks) >= 2:
        out.append(("all", advantage_gate(base, {k: u[k] for k in ks})))
    return out


def mask_of(options, n_vf: int) -> int:
    """The gate mask of SPEC §26.1 for an iterable of option numbers: bit k for each k, 1 <= k < n_vf (ValueError otherwise)."""
    mask = 0
    for k in options:
        k = int(k)
        if not (1 <= k < int(n_vf)):
            raise ValueError(f"mask_of: option {k} is outside 1 .. {int(n_vf) - 1}")
        mask |= 1 << k
    return mask


def nonzero_options(gate) -> list:
    """The options k >= 1 whose row of the table differs from all-zero on either side: set_learner_gate's default choice."""
    g = _table(gate)
    return [k for k in range(1, g.shape[0]) if bool((g[k] != 0).any())]
