"""Trajectory — the per-step rows of recorded rollouts and option trials (SPEC §10) and their host-side views; DeviceRecord —
the same rows kept on the device (SPEC §30.1)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._lib import (ROLLOUT_TERM_INTERRUPTED, TRIAL_EPISODE_END, TRIAL_LEFT_INITIATION, TRIAL_SUCCESS, TRIAL_TIMEOUT,
                   Record, RecordStore, ScgError)

TERMS = {0: "", TRIAL_SUCCESS: "SUCCESS", TRIAL_EPISODE_END: "EPISODE_END", TRIAL_LEFT_INITIATION: "LEFT_INITIATION",
         TRIAL_TIMEOUT: "TIMEOUT", ROLLOUT_TERM_INTERRUPTED: "INTERRUPTED"}
HIST_TERMS = 5             # summary()'s term_hist: codes 0 .. 4; INTERRUPTED (SPEC §11) is counted apart
BEGIN_ACTION = 255         # the action of a begin row (SPEC §10)


class Trajectory:
    """Record buffers of SPEC §10 for envs (or trial entries) first .. first+n-1, `rows` rows per launch, plus the rows of the
    launches appended so far, per env, on the host. Device side: `len` [n] int32 and one [rows][n] tensor per field, the
    buffers one launch writes (`c_struct()`); `append()` copies a launch's rows (cut to len) behind the earlier ones."""

    FIELDS = ("x", "y", "vx", "vy", "reward", "action", "done", "vf", "term", "option_id")
    DTYPES = {"x": torch.float32, "y": torch.float32, "vx": torch.float32, "vy": torch.float32, "reward": torch.float32,
              "action": torch.uint8, "done": torch.uint8, "vf": torch.uint8, "term": torch.uint8, "option_id": torch.int8}

    def __init__(self, n: int, rows: int, first: int = 0, device="cpu", fields=FIELDS, n_vf=None):
        self.first, self.n, self.rows = int(first), int(n), int(rows)
        self.n_vf = None if n_vf is None else int(n_vf)   # value functions of the context (root + options), sizes summary()'s lists
        if self.n < 1 or self.rows < 1 or self.first < 0:
            raise ValueError("a record needs n >= 1, rows >= 1 and first >= 0")
        dev = torch.device(device)
        self.fields = tuple(fields)
        if any(f not in self.DTYPES for f in self.fields):
            raise ValueError(f"unknown record field in {self.fields}")
        self.len = torch.zeros(self.n, dtype=torch.int32, device=dev)
        for f in self.FIELDS:
            setattr(self, f, torch.zeros((self.rows, self.n), dtype=self.DTYPES[f], device=dev) if f in self.fields else None)
        self._chunks = [[] for _ in range(self.n)]       # per env: one dict of numpy rows per appended launch

    @property
    def device(self) -> torch.device:
        return self.len.device

    def c_struct(self) -> Record:
        """The scg_record of these buffers (device pointers; the tensors must stay alive while it is in use)."""
        p = {f: C.c_void_p(getattr(self, f).data_ptr()) for f in self.fields}
        return Record(first=self.first, n=self.n, rows=self.rows, len=C.c_void_p(self.len.data_ptr()), **p)

    def append(self, launch=None) -> "Trajectory":
        """Append one launch's rows: `launch` maps "len" ([n]) and the recorded fields ([rows][n]) to tensors or arrays;
        default: this trajectory's own buffers, as the last launch left them. Each env's first len rows go behind its
        earlier ones."""
        if launch is None:
            launch = {f: getattr(self, f) for f in ("len",) + self.fields}
        host = {f: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for f, v in launch.items()}
        ln = host["len"].astype(np.int64)
        if ln.shape != (self.n,):
            raise ValueError(f"len must hold {self.n} entries")
        for r in range(self.n):
            if ln[r] > 0:
                self._chunks[r].append({f: host[f][: ln[r], r].copy() for f in self.fields})
        return self

    def per_env(self, i: int) -> dict:
        """Env first + i's appended rows: one numpy array per recorded field, all of one length."""
        ch = self._chunks[int(i)]
        return {f: np.concatenate([c[f] for c in ch]) if ch else np.zeros(0, _np_dtype(self.DTYPES[f])) for f in self.fields}

    def length(self, i: int) -> int:
        return int(sum(len(c[self.fields[0]]) for c in self._chunks[int(i)]))

    def segments(self, i: int) -> list:
        """Runs of rows of env i under one value function: dicts with vf, start and end (row indices, inclusive), steps, the
        last row's term and done (0 for a begin row). A run also ends after a row whose option ended (term != 0) and after an episode's last
        step (done != 0 on a row that is not a begin row). Runs under the root are kept; a declined offer shows as root
        rows with option_id < 0. Needs the vf, term, done and action fields."""
        e = self.per_env(i)
        vf, term, done, act = e["vf"], e["term"], e["done"], e["action"]
        out, start = [], 0
        for j in range(len(vf)):
            last = (j + 1 == len(vf) or vf[j + 1] != vf[j] or term[j] != 0
                    or (done[j] != 0 and act[j] != BEGIN_ACTION))
            if last:
                out.append({"vf": int(vf[j]), "start": start, "end": j, "steps": j - start + 1, "term": int(term[j]),
                            "done": int(done[j]) if act[j] != BEGIN_ACTION else 0})
                start = j + 1
        return out

    def describe(self, i: int) -> str:
        """One line per env: its segments in order, e.g. `root×12 → 3×40 SUCCESS → 1×9 EPISODE_END(goal)`; the begin row
        counts with the root segment it opens."""
        parts = []
        for s in self.segments(i):
            name = "root" if s["vf"] == 0 else str(s["vf"])
            txt = f"{name}×{s['steps']}"
            if s["term"]:
                txt += " " + TERMS[s["term"]]
            if s["done"] and not s["term"]:
                txt += " EPISODE_END"
            if s["done"] == 1:
                txt += "(goal)"
            parts.append(txt)
        return " → ".join(parts)

    def summary(self) -> dict:
        """Over all envs, on the host in float64: per value function k (index 0 = the root) the number of segments, their mean
        length in steps (begin rows not counted; NaN without a segment) and the histogram of their terminating term (index =
        code), with one entry per value function of the context (n_vf given at construction; else up to the largest vf seen);
        declined_rows: rows with option_id < 0, i.e. steps that end outside an option whose initiation set holds the next state, its
        offer declined by the value gate or not re-offered yet (a declined offer stays negative over several rows, so
        this is not evaluate()'s count of value-gate declines); episodes (steps with done != 0), goals and goal_rate. Only
        when some segment ends in INTERRUPTED (SPEC §11): interrupted, those segments per value function (not in term_hist)."""
        seen = 1 + max([int(s["vf"]) for i in range(self.n) for s in self.segments(i)] + [0])
        n_vf = seen if self.n_vf is None else max(self.n_vf, seen)
        seg = np.zeros(n_vf, np.int64)
        steps = np.zeros(n_vf, np.float64)
        hist = np.zeros((n_vf, HIST_TERMS), np.int64)
        intr = np.zeros(n_vf, np.int64)
        episodes = goals = declined_rows = 0
        for i in range(self.n):
            e = self.per_env(i)
            real = e["action"] != BEGIN_ACTION
            for s in self.segments(i):
                k = s["vf"]
                seg[k] += 1
                steps[k] += float(np.sum(real[s["start"]: s["end"] + 1]))
                if s["term"] == ROLLOUT_TERM_INTERRUPTED:
                    intr[k] += 1
                else:
                    hist[k, s["term"]] += 1
            episodes += int(np.sum((e["done"] != 0) & real))
            goals += int(np.sum((e["done"] == 1) & real))
            if "option_id" in e:
                declined_rows += int(np.sum(e["option_id"] < 0))
        nan = float("nan")
        out = {
            "segments": [int(v) for v in seg],
            "mean_steps": [float(steps[k] / seg[k]) if seg[k] else nan for k in range(n_vf)],
            "term_hist": [[int(v) for v in hist[k]] for k in range(n_vf)],
            "declined_rows": declined_rows,
            "episodes": episodes,
            "goals": goals,
            "goal_rate": goals / episodes if episodes else nan,
        }
        if intr.any():
            out["interrupted"] = [int(v) for v in intr]
        return out

    def resume_state(self, env, row) -> dict:
        """SPEC §19.2: the env state a one-episode record's env `env[i]` was in BEFORE step `row[i]` (row 0 is its begin row, so
        row >= 1), exactly as the kernel held it — what a branch rollout resumes. Host arrays, one entry per (env, row):
          x, y, vx, vy, option_id   of row - 1 (the begin row holds the start state; a row that ends no episode has no reset)
          ep_steps                  row - 1
          opt_steps                 the recurrence the kernel runs over rows 0 .. row - 1: 0 after the begin row, prev + 1 after a
                                    row with vf >= 1 and term == 0 (the option goes on), otherwise 0 (an interrupted row has term 5)
          vf_next                   the value function that runs step `row`: option_id if 1 <= option_id < n_vf, else 0
        plus env and row as given. Needs the state fields, vf, term, done, action and option_id, and n_vf (given at construction).
        Raises ValueError for a row < 1 or at or beyond the env's length, and where row - 1 ended the episode (done != 0 on a row
        that is not the begin row): the state after that row is the next episode's drawn start, which the record does not hold."""
        need = ("x", "y", "vx", "vy", "vf", "term", "done", "action", "option_id")
        if any(f not in self.fields for f in need) or self.n_vf is None:
            raise ValueError(f"resume_state needs the record fields {need} and n_vf")
        env, row = np.asarray(env, np.int64).reshape(-1), np.asarray(row, np.int64).reshape(-1)
        if env.shape != row.shape:
            raise ValueError("env and row must have one length")
        if np.any(env < 0) or np.any(env >= self.n):
            raise ValueError(f"env outside the record's {self.n} envs")
        out = {"x": np.zeros(len(env), np.float32), "y": np.zeros(len(env), np.float32), "vx": np.zeros(len(env), np.float32),
               "vy": np.zeros(len(env), np.float32), "option_id": np.zeros(len(env), np.int32), "opt_steps": np.zeros(len(env), np.int32),
               "ep_steps": (row - 1).astype(np.int32), "env": env, "row": row}
        for e in np.unique(env):
            at = np.nonzero(env == e)[0]
            rec, r = self.per_env(e), row[at]
            n = len(rec["vf"])
            if np.any(r < 1) or np.any(r >= n):
                raise ValueError(f"env {int(e)}: row outside 1 .. {n - 1} (the record holds {n} rows of it)")
            ended = (rec["done"][r - 1] != 0) & (rec["action"][r - 1] != BEGIN_ACTION)
            if np.any(ended):
                raise ValueError(f"env {int(e)}: row {int(r[ended][0]) - 1} ended the episode: there is no state to resume behind it")
            goes_on = (rec["vf"] >= 1) & (rec["term"] == 0)       # (the begin row: vf = 0)
            j = np.arange(n)
            last_reset = np.maximum.accumulate(np.where(goes_on, -1, j))      # the last row <= j that left opt_steps at 0
            for f in ("x", "y", "vx", "vy"):
                out[f][at] = rec[f][r - 1]
            out["option_id"][at] = rec["option_id"][r - 1]
            out["opt_steps"][at] = (j - last_reset)[r - 1]
        oid = out["option_id"].astype(np.int64)
        out["vf_next"] = np.where((oid >= 1) & (oid < self.n_vf), oid, 0)
        return out

    def offer_rows(self, reoffer_period: int = 1, t0: int = 0, env_ids=None) -> dict:
        """The recorded rows on which the root ran, the episode went on and an option was offered or stayed out of (vf = 0,
        done = 0, option_id != 0), in env order: host arrays `flat` (the row's index in to_numpy()'s concatenated fields), `env`,
        `row`, `option` (|option_id|: the candidate), `entered` (option_id > 0) and `stay`. On such a row the recorded state is
        s_next, the state §4.2's value gate compared at (an episode's last row holds the state before its reset instead, and is
        left out). A row is a `stay` where §4.2's re-offer schedule kept the env out of the option the row before it left it out
        of — the id unchanged and negative, and ((t + env id) & (reoffer_period - 1)) != 0 with t = t0 + row (`t0`: the step
        counter of each env's row 0; `env_ids`: the envs' global ids, default first .. first + n - 1): no offer was made there
        and the gate compared nothing. Every other row is an offer whose outcome the sign of the id records. With the default
        period of 1 every row is an offer. Needs the vf, done and option_id fields."""
        return offer_rows(self.to_numpy(), reoffer_period, t0, env_ids)

    def offer_states(self, limit=None):
        """(x, y, vx, vy), float32 host arrays, of the first `limit` rows of offer_rows() in env order (None: all of them; the rows
        an env stayed out of an option on are among them): states at which offers actually happen, for gate_audit(states=)."""
        return offer_states(self.to_numpy(), limit)

    def to_numpy(self) -> dict:
        """Every env's rows flattened for saving: `offsets` [n + 1] into the concatenated fields, plus `first`."""
        per = [self.per_env(i) for i in range(self.n)]
        off = np.zeros(self.n + 1, np.int64)
        off[1:] = np.cumsum([len(p[self.fields[0]]) for p in per])
        out = {f: np.concatenate([p[f] for p in per]) for f in self.fields}
        out["offsets"], out["first"] = off, np.int64(self.first)
        return out


class DeviceRecord:
    """SPEC §30.1's device store of a record: for `n` envs with room for `cap` rows each one [n][cap] tensor per recorded field,
    `have` [n] (int32: rows held) and `overflow` [1] (int32: rows dropped because they passed cap), all on `ctx`'s device. What
    Trajectory keeps on the host, kept where the launches write it: append() is one scg_record_append call, flat() gives the
    record in (env, row) order — Trajectory.to_numpy()'s layout — as device tensors, with the row tables of the value fits."""

    TABLES = ("env", "row", "tab0", "tabk", "tabA")
    _TABLE_DTYPES = {"env": torch.int32, "row": torch.int32, "tab0": torch.uint8, "tabk": torch.uint8, "tabA": torch.uint8}

    def __init__(self, ctx, n: int, cap: int, first: int = 0, fields=Trajectory.FIELDS, n_vf=None):
        self.ctx, self.first, self.n, self.cap = ctx, int(first), int(n), int(cap)
        self.n_vf = None if n_vf is None else int(n_vf)
        if self.n < 1 or self.cap < 1 or self.first < 0:
            raise ValueError("a device record needs n >= 1, cap >= 1 and first >= 0")
        self.fields = tuple(fields)
        if any(f not in Trajectory.DTYPES for f in self.fields):
            raise ValueError(f"unknown record field in {self.fields}")
        dev = ctx.device
        for f in Trajectory.FIELDS:
            setattr(self, f, torch.empty((self.n, self.cap), dtype=Trajectory.DTYPES[f], device=dev) if f in self.fields else None)
        self.have = torch.zeros(self.n, dtype=torch.int32, device=dev)
        self.overflow = torch.zeros(1, dtype=torch.int32, device=dev)
        self._flat = None

    @property
    def device(self) -> torch.device:
        return self.have.device

    def c_struct(self) -> RecordStore:
        """The scg_record_store of these tensors (device pointers; the tensors must stay alive while it is in use)."""
        p = {f: C.c_void_p(getattr(self, f).data_ptr()) for f in self.fields}
        return RecordStore(have=C.c_void_p(self.have.data_ptr()), overflow=C.c_void_p(self.overflow.data_ptr()), **p)

    def append(self, launch: Trajectory) -> "DeviceRecord":
        """Append the rows the last launch left in `launch`'s buffers (a Trajectory of the same n on this device; its host rows
        are not touched): one scg_record_append call on the current stream, no download and no loop over the envs."""
        if not isinstance(launch, Trajectory) or launch.n != self.n or launch.device != self.device:
            raise ScgError(f"DeviceRecord.append: the launch buffers must be a Trajectory of {self.n} envs on {self.device}")
        self.ctx.record_append(launch.c_struct(), self.c_struct(), self.cap)
        self._flat = None
        return self

    @classmethod
    def from_trajectory(cls, ctx, traj: Trajectory) -> "DeviceRecord":
        """A host Trajectory's appended rows as a device record: one upload per field."""
        flat = traj.to_numpy()
        off = flat["offsets"]
        L = np.diff(off)
        rec = cls(ctx, traj.n, max(int(L.max()), 1), traj.first, traj.fields, traj.n_vf)
        env = np.repeat(np.arange(traj.n), L)
        row = np.arange(int(off[-1])) - off[:-1][env]
        for f in rec.fields:
            host = np.zeros((rec.n, rec.cap), flat[f].dtype)
            host[env, row] = flat[f]
            getattr(rec, f).copy_(torch.from_numpy(host))
        rec.have.copy_(torch.from_numpy(L.astype(np.int32)))
        return rec

    def flat(self, ctx=None) -> dict:
        """The record in (env, row) order as device tensors: `offsets` (int64 [n + 1]), one [total] tensor per recorded field, `env`
        and `row` (int32) and, where done, vf and term are recorded, `tab0`, `tabk`, `tabA` (uint8: SPEC §30.1's row tables); plus
        `total` (int). scg_record_offsets, ONE read-back (offsets[n] and overflow), scg_record_pack; cached until the next append.
        `ctx`: the context that makes the calls (default: the one given at construction; any live context of the device serves).
        Raises ScgError where rows were dropped: the record is not the episodes'."""
        if self._flat is not None:
            return self._flat
        ctx = self.ctx if ctx is None else ctx
        off = ctx.record_offsets(self.have)
        total, dropped = (int(v) for v in torch.cat([off[-1:], self.overflow.to(torch.int64)]).cpu())
        if dropped:
            raise ScgError(f"DeviceRecord: {dropped} rows passed the capacity of {self.cap} rows per env and were dropped")
        dev = self.device
        out = {f: torch.empty(total, dtype=Trajectory.DTYPES[f], device=dev) for f in self.fields}
        names = self.TABLES if all(f in self.fields for f in ("done", "vf", "term")) else self.TABLES[:2]
        extra = {f: torch.empty(total, dtype=self._TABLE_DTYPES[f], device=dev) for f in names}
        ctx.record_pack(self.n, self.cap, self.c_struct(), off, total, out, extra)
        self._flat = {"offsets": off, "total": total, **out, **extra}
        return self._flat

    def to_numpy(self) -> dict:
        """Trajectory.to_numpy()'s dict of this record, equal by bits."""
        fl = self.flat()
        out = {f: fl[f].cpu().numpy() for f in self.fields}
        out["offsets"], out["first"] = fl["offsets"].cpu().numpy(), np.int64(self.first)
        return out

    def to_trajectory(self) -> Trajectory:
        """The record as a host Trajectory (no launch buffers to speak of), for the host-side views: segments, summary,
        resume_state, offer_rows."""
        flat = self.to_numpy()
        off = flat["offsets"]
        traj = Trajectory(self.n, 1, self.first, "cpu", self.fields, self.n_vf)
        for e in range(self.n):
            if off[e + 1] > off[e]:
                traj._chunks[e].append({f: flat[f][off[e]: off[e + 1]].copy() for f in self.fields})
        return traj


def offer_rows(flat: dict, reoffer_period: int = 1, t0: int = 0, env_ids=None) -> dict:
    """Trajectory.offer_rows on to_numpy()'s dict `flat` (without `offsets`: the rows of one env, `first` 0)."""
    period = int(reoffer_period)
    if period < 1 or period & (period - 1):
        raise ValueError("reoffer_period must be a power of two >= 1")
    oid = np.asarray(flat["option_id"]).astype(np.int64)
    off = np.asarray(flat.get("offsets", [0, len(oid)]), np.int64)
    n = len(off) - 1
    ids = int(flat.get("first", 0)) + np.arange(n, dtype=np.int64) if env_ids is None else np.asarray(env_ids, np.int64).reshape(-1)
    if ids.shape != (n,):
        raise ValueError(f"env_ids must hold {n} entries")
    at = np.nonzero((np.asarray(flat["vf"]) == 0) & (np.asarray(flat["done"]) == 0) & (oid != 0))[0]
    env = np.searchsorted(off, at, side="right") - 1
    row = at - off[env]
    prev = np.where(row > 0, oid[np.maximum(at - 1, 0)], 0)    # the id the step came in with (an env's row 0: none)
    off_schedule = ((int(t0) + row + ids[env]) & (period - 1)) != 0
    return {"flat": at, "env": env, "row": row, "option": np.abs(oid[at]), "entered": oid[at] > 0,
            "stay": (oid[at] < 0) & (prev == oid[at]) & off_schedule}


def offer_states(flat: dict, limit=None):
    """Trajectory.offer_states on to_numpy()'s dict."""
    at = offer_rows(flat)["flat"][:limit]
    return tuple(np.ascontiguousarray(np.asarray(flat[f])[at], np.float32) for f in ("x", "y", "vx", "vy"))


def _np_dtype(dt: torch.dtype):
    return torch.empty(0, dtype=dt).numpy().dtype
