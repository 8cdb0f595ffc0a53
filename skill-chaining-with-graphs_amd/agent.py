"""SkillChainingAgent — host driver of the fused step-batch (SPEC.md §4–§5).

north_star names `SkillChainingAgent.q_update` and asks that the Option / SkillChainingAgent Python API
be kept; the reference holds no code (README.md:1-2 only), so the API below is this build's own,
named after north_star. Per-step work is one scg_step launch pair (fused kernel + reduce/apply);
nothing on the per-step path synchronises with or copies to the host."""
from __future__ import annotations

import contextlib
import functools
import os
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from . import dist as _dist
from . import gatefit
from . import initfit
from ._lib import CLF_STRIDE, NUM_ACTIONS, NUM_FEATURES, ScgError, auto_block_envs
from .core import EnvState, ScgContext
from .evaluation import BranchResult, EpisodeStats, GateAudit, paired_differences
from .maps import PinballMap, load_map
from .option import Option
from .pinball import PinballDomain
from .trajectory import DeviceRecord, Trajectory
from .trials import OUTCOMES, TrialResult


def frontier_masks(k: int, enabled_mask: int, gest_mask: int, parents, max_children: Optional[int] = None):
    """SPEC §13's nodes for creating option k: (target_mask, cover_mask). Targets: the goal (node 0) and every enabled,
    not gestating option j < k that fewer than `max_children` known options target already (None: no cap). Cover: every
    known option (enabled | gest). parent[k] < k keeps the graph acyclic by construction."""
    known = (enabled_mask | gest_mask) & ~1
    target = 1
    for j in range(1, k):
        if not ((enabled_mask >> j) & 1) or (gest_mask >> j) & 1:
            continue
        children = sum(1 for i in range(1, len(parents)) if (known >> i) & 1 and int(parents[i]) == j)
        if max_children is None or children < max_children:
            target |= 1 << j
    return target, known


def choose_parent(counts, target_mask: int, min_examples: int) -> Optional[int]:
    """SPEC §13: the target node holding the most examples (ties: the lower node id), or None when it holds fewer than
    `min_examples` (growth stops)."""
    best = None
    for p, c in enumerate(counts):
        if (target_mask >> p) & 1 and (best is None or c > counts[best]):
            best = p
    return best if best is not None and counts[best] >= min_examples else None


class SkillChainingAgent:
    def __init__(self, pmap, n_envs: int, n_options: int = 0, *, device: int = 0, seed: int = 0,
                 env_id_base: int = 0, group=None, ordered_sum: bool = False, transport: str = "collective",
                 interrupt_learning: bool = False, **hparams):
        # transport (shared weights only): "collective" = a torch.distributed collective per learning step-batch; "peer" = the
        # ranks of one node read each other's operands through HIP IPC and sum them in rank order on the device
        if transport not in ("collective", "peer"):
            raise ValueError("transport must be 'collective' or 'peer'")
        if transport == "peer" and (group is None or not ordered_sum):
            raise ValueError("transport='peer' needs group=... and ordered_sum=True (it is a transport of the order-pinned sum)")
        self.map: PinballMap = load_map(pmap) if isinstance(pmap, str) else pmap
        if group is not None and hparams.get("block_envs") is None and not os.environ.get("SCG_BLOCK_ENVS"):
            # a sharded run uses ONE block geometry (it orders the partial sums of G): the ranks agree on the largest any of them
            # would pick from its own env count (equal shards pick equal sizes anyway)
            hparams["block_envs"] = _dist.allreduce_max_int(auto_block_envs(n_envs), group, torch.device("cuda", device))
        self.ctx = ScgContext(n_envs, n_options, self.map, device=device, seed=seed, env_id_base=env_id_base,
                              **hparams)
        dev = self.ctx.device
        self.n_envs, self.n_options, self.n_vf = n_envs, n_options, n_options + 1
        self.W = torch.zeros((self.n_vf, NUM_ACTIONS, NUM_FEATURES), dtype=torch.float32, device=dev)
        self.clf = torch.zeros((self.n_vf, CLF_STRIDE), dtype=torch.float32, device=dev)
        self.enabled_mask = 0
        # SPEC §25.3: the gate table evaluate() / evaluate_policies() act under by default ([n_vf, 2, 5, 1296], gatefit), or None for
        # §4.2's own comparison; stored by improve_gate(apply=True). The learner and every other kernel ignore it; not in state_dict()
        self.gate = None
        # SPEC §26.2: the gate table the LEARNER's step-batches take their entry decisions from (set_learner_gate), with the mask of
        # the options that compare under it, or None for §4.2's own comparison on W. Independent of `gate`; not in state_dict()
        self.learner_gate = None
        self.learner_gate_mask = 0
        self.gest_mask = 0            # SPEC §4.4: options in gestation
        self._gest_need = {}
        self.t = 0
        self.group = group            # torch.distributed group for shared option-Q weights (or None)
        self.ordered_sum = bool(ordered_sum)   # shared weights summed in rank order from an all-gather (identical on every
        self._slots = None                     # rank of the run, reproduced by the oracle) instead of an all-reduce (exact for two ranks)
        self.allreduce_timing = None  # see time_allreduce()
        self.transport = transport
        # SPEC §12: learning step-batches interrupt options (settable between steps; not a part of state_dict(), like the
        # hyper-parameters). Acting-only step-batches never interrupt: evaluate(interrupt=True) does that for acting
        self.interrupt_learning = bool(interrupt_learning)
        if transport == "peer":
            _dist.exchange_peer_handles(self.ctx, group)
        self.domain = PinballDomain(self.ctx)
        self.state: EnvState = self.domain.state
        self.options: List[Option] = [Option(self, k) for k in range(self.n_vf)]
        self.trace, self._ex, self._ex_cap = None, {}, None     # enable_tracing(): the ring + events, the example buffers by option
        # grow_skill_tree()'s per-node buffers (kept for inspection); evaluate()'s n_episodes -> (context, EnvState, EpisodeStats); option_trials()'s context
        self._frontier, self._eval_ctx, self._trial_ctx, self._branch_ctx = None, {}, None, {}

    # ------------------------------------------------------------------ option management (outer loop)
    def enable_option(self, k: int, enabled: bool = True) -> None:
        if not (1 <= k <= self.n_options):
            raise ValueError("option index out of range")
        self.enabled_mask = (self.enabled_mask | (1 << k)) if enabled else (self.enabled_mask & ~(1 << k))

    # ------------------------------------------------------------------ skill discovery (outer loop, SPEC §7)
    def enable_tracing(self, ring_len: int = 256, max_examples: int = 65536) -> None:
        """Attach the device-resident trajectory ring + per-step event flags (costs ~13 B/env-step) and the per-option
        example buffers (max_examples each) the device-side trigger appends to."""
        self.trace = self.ctx.set_trace_buffers(ring_len)
        self._ex_cap = int(max_examples)
        self._ex = {}                     # k -> (xy[cap, 2], label[cap], count[1], prev_in[N] or None), all on the device

    def _ex_buffers(self, k: int):
        if k not in self._ex:
            dev, cap = self.W.device, self._ex_cap
            parent = int(self.ctx.parents[k])
            self._ex[k] = (torch.zeros((cap, 2), dtype=torch.float32, device=dev),
                           torch.zeros(cap, dtype=torch.uint8, device=dev),
                           torch.zeros(1, dtype=torch.int32, device=dev),
                           torch.zeros(self.n_envs, dtype=torch.uint8, device=dev) if parent else None)
        return self._ex[k]

    def collect_examples(self, k: int, l_pos: int = 32, l_neg: int = 32) -> None:
        """Call after a step_batch while option k is being created: envs whose step ended inside option k's target
        region (goal disc if parent[k] = 0, else the parent's initiation set, on the step they ENTER it) append their
        last l_pos ring states as positives and the l_neg states before those as negatives to option k's example
        buffer. Selection, compaction and the gather run on the device (SPEC §7; one launch behind the step, whose
        commit rows leave the row totals of the announced trigger): nothing is read back, the host is not in the
        per-step path; examples_held(k) fetches the count when the outer loop wants it."""
        xy, lab, cnt, prev = self._ex_buffers(k)
        parent = int(self.ctx.parents[k])
        self.ctx.collect_examples(1 if parent == 0 else (1 << parent), prev, l_pos, l_neg, xy.view(-1), lab, cnt)

    def examples_held(self, k: int) -> int:
        """Examples in option k's buffer (one device->host read; node-wide total when the agent is sharded, so that
        every rank takes the same branch in the outer loop)."""
        got = int(self._ex_buffers(k)[2].item())
        if self.group is not None:
            got = _dist.allreduce_sum_int(got, self.group, self.W.device)
        return got

    def examples(self, k: int):
        """(xy[n, 2], label[n]) collected for option k so far (views of the device buffers)."""
        xy, lab, cnt, _ = self._ex_buffers(k)
        n = int(cnt.item())
        return xy[:n], lab[:n]

    def create_option(self, k: int, iters: int = 400, lr: float = 3.0, l2: float = 1e-4, gestation: int = 0) -> float:
        """Fit initiation classifier k on the collected examples (GPU logistic regression) and start its value function
        from the root's. With gestation = 0 the option is enabled at once; with gestation = G > 0 it first gestates
        (SPEC §4.4, Konidaris & Barto 2009): its classifier is in use, it is never selected, every transition from inside
        its initiation set updates its value function off-policy, and poll_gestation() enables it once G such
        transitions have reached its target. Returns the training accuracy."""
        self.ctx.disarm_collect()            # the collection for this option is over
        xy, lab = self.examples(k)
        if self.group is not None:           # fit on the examples of ALL ranks (rank order): identical classifiers everywhere
            xy, lab = _dist.allgather_rows(xy.contiguous(), self.group), _dist.allgather_rows(lab.contiguous(), self.group)
        clf = self.options[k].initiation_classifier
        err = None
        try:
            clf.fit(xy.contiguous(), lab.contiguous(), iters=iters, lr=lr, l2=l2)
        except ScgError as e:                # the fit gave up on the device (sticky status word): the row is untouched
            err = e
        if self.group is not None:           # a give-up is rank-local: agree on it before anyone acts on the classifier,
            bad = _dist.allreduce_sum_int(1 if err else 0, self.group, self.W.device)      # or the peers hang in the next collective
            if bad and err is None:
                raise ScgError(f"create_option({k}): the initiation-set fit gave up on {bad} other rank(s); no rank enables the option")
        if err is not None:
            raise err
        self.W[k].copy_(self.W[0])
        if gestation > 0:
            self._gest_need[k] = int(gestation)
            self.gest_mask |= 1 << k
            succ = self.ctx.set_gestation(self.gest_mask)
            succ[k] = 0
        else:
            self.enable_option(k)
        pred = clf.predict(xy[:, 0].contiguous(), xy[:, 1].contiguous())
        return float((pred == lab).float().mean())

    def poll_gestation(self) -> list:
        """Enable every gestating option whose success count has reached its requirement (one device->host read;
        counts are summed over the ranks of a sharded agent). Returns the options enabled by this call."""
        if not self.gest_mask:
            return []
        succ = self.ctx.set_gestation(self.gest_mask).cpu()
        done = []
        for k in range(1, self.n_options + 1):
            if not (self.gest_mask >> k) & 1:
                continue
            n = int(succ[k])
            if self.group is not None:
                n = _dist.allreduce_sum_int(n, self.group, self.W.device)
            if n >= self._gest_need[k]:
                self.gest_mask &= ~(1 << k)
                self.enable_option(k)
                done.append(k)
        if done:
            self.ctx.set_gestation(self.gest_mask)
        return done

    def chain_skills(self, steps_per_option: int = 300, min_examples: int = 2000, max_examples: int = 40000,
                     l_pos: int = 24, l_neg: int = 24, start_coverage: float = 0.5, poll_every: int = 8,
                     gestation: int = 0, gestation_steps: int = 200, **fit) -> list:
        """The outer loop of skill chaining (Konidaris & Barto 2009, the paper README.md:2 names), host-side
        policy over the device-resident pieces: for each not-yet-enabled option k in index order, run
        step-batches until enough trajectories have entered k's target (its parent in the skill graph),
        fit initiation set k on them, let it gestate (`gestation` successes, at most `gestation_steps` step-batches)
        or enable it at once, and stop once the start states are covered. The host looks at the device-side
        counters only every `poll_every` step-batches. Returns one report dict per created option."""
        report = []
        max_examples = min(max_examples, self._ex_cap)
        for k in range(1, self.n_options + 1):
            if ((self.enabled_mask | self.gest_mask) >> k) & 1:
                continue
            got, steps = self._collect_until(lambda: self.collect_examples(k, l_pos, l_neg), lambda: self.examples_held(k),
                                             lambda got: got >= max_examples, 0, steps_per_option, poll_every)
            if got < min_examples:
                break
            acc, gsteps = self._fit_and_gestate(k, gestation, gestation_steps, poll_every, fit)
            cov = self._start_coverage([k])
            report.append(dict(option=k, parent=int(self.ctx.parents[k]), steps=steps, examples=got,
                               accuracy=acc, start_coverage=cov, gestation_steps=gsteps))
            if cov >= start_coverage:
                break
        return report

    def _collect_until(self, collect, held, full, counts, steps_per_option: int, poll_every: int):
        """An option's collection in chain_skills and grow_skill_tree: step-batches with `collect()` behind each, until
        `steps_per_option` of them have run or `full(counts)`; the host reads `held()`, the counts (from `counts` on), and
        the gestation counters only every `poll_every` step-batches. Returns (counts, step-batches run)."""
        steps = 0
        while steps < steps_per_option and not full(counts):
            for _ in range(min(poll_every, steps_per_option - steps)):
                self.step_batch()
                collect()
                steps += 1
            counts = held()
            self.poll_gestation()
        return counts, steps

    def _start_coverage(self, options) -> float:
        """The share of the map's start states that lie in the initiation set of one of `options`."""
        sx, sy = (torch.as_tensor(self.map.starts[:, i].copy(), device=self.W.device) for i in (0, 1))
        inside = torch.zeros_like(sx, dtype=torch.bool)
        for j in options:
            inside |= self.options[j].initiation_classifier.predict(sx, sy).bool()
        return float(inside.float().mean())

    def _fit_and_gestate(self, k: int, gestation: int, gestation_steps: int, poll_every: int, fit: dict):
        """Fit option k on its example buffer (create_option) and run its gestation: step-batches until the success counters
        enable it, at most `gestation_steps` of them, then enable it anyway. Returns (training accuracy, gestation step-batches)."""
        acc = self.create_option(k, gestation=gestation, **fit)
        gsteps = 0
        while (self.gest_mask >> k) & 1 and gsteps < gestation_steps:
            for _ in range(poll_every):
                self.step_batch()
            gsteps += poll_every
            self.poll_gestation()
        if (self.gest_mask >> k) & 1:            # did not see enough successes: enable anyway, as the paper's
            self.gest_mask &= ~(1 << k)          # fixed-length gestation period would
            self.ctx.set_gestation(self.gest_mask)
            self.enable_option(k)
        return acc, gsteps

    def grow_skill_tree(self, steps_per_option: int = 300, min_examples: int = 2000, max_examples: int = 40000,
                        l_pos: int = 24, l_neg: int = 24, start_coverage: float = 0.5, poll_every: int = 8,
                        max_children: Optional[int] = None, gestation: int = 0, gestation_steps: int = 200, **fit) -> list:
        """Skill-tree discovery (SPEC §13; the extension Konidaris & Barto 2009 discuss): like chain_skills, but a new option
        may target the goal or ANY enabled option, not only the one created last. For each free option index k in order,
        step-batches run with the device-side frontier collection behind each (one buffer per node of the graph: envs that
        enter a target node from territory no known option covers), until `steps_per_option` step-batches have run or a
        node holds `max_examples`; the host reads the per-node counts every `poll_every` step-batches. The node holding the
        most examples (ties: the lower id) becomes parent[k]; below `min_examples` growth stops. Option k is fitted on that
        node's rows (they become its example buffer: examples(k), state_dict()), started from the root's weights and
        gestated exactly as in chain_skills. Growth stops once the union of the known options' initiation sets covers
        `start_coverage` of the map's start states. `max_children` caps the options that may target one option (None: no
        cap). Returns one report dict per created option."""
        if self.group is not None:
            raise ValueError("grow_skill_tree: a sharded agent (group=...) cannot grow a skill tree yet; use chain_skills")
        if self.trace is None:
            raise ScgError("grow_skill_tree: tracing is off (enable_tracing)")
        dev = self.W.device
        cap = min(max_examples, self._ex_cap)
        node_xy = torch.zeros((self.n_vf, cap, 2), dtype=torch.float32, device=dev)
        node_lab = torch.zeros((self.n_vf, cap), dtype=torch.uint8, device=dev)
        node_cnt = torch.zeros(self.n_vf, dtype=torch.int32, device=dev)
        self._frontier = (node_xy, node_lab, node_cnt)
        report = []
        for k in range(1, self.n_options + 1):
            if ((self.enabled_mask | self.gest_mask) >> k) & 1:
                continue
            target, cover = frontier_masks(k, self.enabled_mask, self.gest_mask, self.ctx.parents, max_children)
            node_cnt.zero_()
            counts, steps = self._collect_until(
                lambda: self.ctx.collect_frontier(target, cover, self.clf.view(-1), l_pos, l_neg, node_xy.view(-1),
                                                  node_lab.view(-1), node_cnt),
                lambda: [int(c) for c in node_cnt.tolist()],
                lambda counts: max(counts[p] for p in range(self.n_vf) if (target >> p) & 1) >= cap,
                [0] * self.n_vf, steps_per_option, poll_every)
            p = choose_parent(counts, target, min_examples)
            if p is None:
                break
            parents = self.ctx.parents.copy()
            parents[k] = p
            self.set_option_parents(parents)
            self._ex.pop(k, None)                   # option k's buffer now belongs to its new parent
            xy, lab, cnt, _ = self._ex_buffers(k)
            n = counts[p]
            xy[:n].copy_(node_xy[p, :n]); lab[:n].copy_(node_lab[p, :n]); cnt.fill_(n)
            acc, gsteps = self._fit_and_gestate(k, gestation, gestation_steps, poll_every, fit)
            known = self.enabled_mask | self.gest_mask
            cov = self._start_coverage([j for j in range(1, self.n_options + 1) if (known >> j) & 1])
            report.append(dict(option=k, parent=p, steps=steps, examples=n, node_examples=counts, accuracy=acc,
                               start_coverage=cov, gestation_steps=gsteps))
            if cov >= start_coverage:
                break
        return report

    # ------------------------------------------------------------------ the skill graph (SPEC §4.2)
    def set_option_parents(self, parents) -> None:
        """parents[k] = the option whose initiation set option k chains to (0 = task goal); entry 0 ignored.
        The default is a chain; any acyclic assignment gives a skill tree rooted at the goal."""
        self.ctx.set_option_parents(parents)

    def skill_graph(self):
        """networkx.DiGraph of the discovered skills: node 0 = task goal, node k = option k (attrs: enabled,
        classifier weights), edge k -> parent[k] = "executing k leads into the initiation set of parent"."""
        import networkx as nx
        g = nx.DiGraph()
        g.add_node(0, kind="goal", target=tuple(self.map.target))
        clf = self.clf.cpu().numpy()
        for k in range(1, self.n_options + 1):
            g.add_node(k, kind="option", enabled=bool((self.enabled_mask >> k) & 1), classifier=clf[k, :6].tolist())
            g.add_edge(k, int(self.ctx.parents[k]))
        return g

    def init_weights(self, std: float = 1e-3, seed: int = 0) -> None:
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.W.copy_(torch.randn(self.W.shape, generator=g) * std)

    # ------------------------------------------------------------------ SPEC §26.2: the learner's gate table
    def _chk_learner_gate(self) -> None:
        if self.group is not None:
            raise ValueError("a learner gate is not available on a sharded agent (the table would have to be identical on every rank)")
        if self.interrupt_learning:
            raise ValueError("a learner gate with interrupt_learning=True is not defined (SPEC §26.1)")

    def set_learner_gate(self, table, options=None) -> None:
        """Let every following step_batch (learning or acting, chain_skills / grow_skill_tree included) take the entry decisions of
        `options` from the gate table `table` ([n_vf, 2, 5, 1296], gatefit's layout) instead of from §4.2's comparison on W; every
        other option keeps that comparison, and nothing else about the step changes (SPEC §26). `options` is an iterable of option
        numbers; the default is every option whose row of `table` differs from all-zero on either side (so a table built by
        gatefit.advantage_gate over gatefit.always_enter masks exactly the fitted options; for gatefit.always_enter itself, whose
        rows are all zero, name the options). set_learner_gate(None) clears it. The table is copied to the agent's device and
        kept as `learner_gate`, the mask as `learner_gate_mask`; `gate`, the evaluation gate, is independent and unchanged.
        ValueError on a sharded agent, with interrupt_learning=True, for a misshapen table or an option outside 1 .. n_options."""
        if table is None:
            self.learner_gate, self.learner_gate_mask = None, 0
            return
        self._chk_learner_gate()
        g = torch.as_tensor(table, dtype=torch.float32)
        if tuple(g.shape) != (self.n_vf, 2, NUM_ACTIONS, NUM_FEATURES):
            raise ValueError(f"set_learner_gate: the table must be [{self.n_vf}, 2, {NUM_ACTIONS}, {NUM_FEATURES}], not {tuple(g.shape)}")
        if options is None:
            options = gatefit.nonzero_options(g)
        mask = gatefit.mask_of(options, self.n_vf)
        self.learner_gate = g.to(self.ctx.device).contiguous().clone()
        self.learner_gate_mask = mask

    # ------------------------------------------------------------------ the hot path
    def step_batch(self, learn: bool = True) -> None:
        """One fused step-batch over all envs (act, physics, options, features, Q, TD, update). A learning step-batch interrupts
        options when `interrupt_learning` is set (SPEC §12); an acting-only one (learn=False) never does — evaluate(interrupt=True)
        is the acting counterpart."""
        shared = self.group is not None and learn
        if shared and self.transport != "peer":
            gp = self.ctx.grad_packed()                  # G and the update counts: ONE all-reduce operand
        if self.learner_gate is not None:                # SPEC §26.2: the masked options' entry decisions come from the table
            self._chk_learner_gate()
            self.ctx.step(self.state, self.W, self.clf, self.enabled_mask, self.t, learn=learn, apply=not shared,
                          gate=self.learner_gate, gate_mask=self.learner_gate_mask)
        else:
            self.ctx.step(self.state, self.W, self.clf, self.enabled_mask, self.t, learn=learn, apply=not shared,
                          interrupt=learn and self.interrupt_learning)
        if shared and self.transport == "peer":
            # the step left the operand in this rank's peer region: ONE call publishes it, waits for every rank's and applies their sum
            try:
                with self._exchange_timed():
                    self.ctx.peer_exchange_apply(self.W)
            finally:
                self.t += 1
            return
        if shared:                                       # (nested: an unshared step-batch pays one test here, not two)
            if self.ordered_sum:
                if self._slots is None:
                    import torch.distributed as dist
                    self._slots = torch.zeros((dist.get_world_size(self.group), gp.numel()), dtype=torch.float32, device=gp.device)
                with self._exchange_timed():
                    _dist.allgather_packed(gp, self._slots, self.group)     # one all-gather; the sum is taken in rank order on every rank
                self.ctx.apply_update_slots(self.W, self._slots)
            else:
                with self._exchange_timed():
                    _dist.allreduce_packed(gp, self.group)      # RCCL over xGMI: one latency-bound 26 KB x n_vf message
                self.ctx.apply_update_packed(self.W, gp)
        self.t += 1

    @contextlib.contextmanager
    def _exchange_timed(self):
        """Around a step-batch's exchange: time_allreduce()'s event pair on the stream of use, when it samples this step (bench.py)."""
        timing = self.allreduce_timing
        if timing is None or (self.t % timing["every"]) != 0:
            yield
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        try:
            yield
        finally:
            e1.record()
            timing["events"].append((e0, e1))

    def time_allreduce(self, every: int = 0) -> Optional[dict]:
        """every > 0: bracket every `every`-th shared-weights all-reduce with an event pair on the current stream
        (what the step's stream waits for: the collective as the step sees it, exposed). every = 0: stop and return
        {"samples", "mean_us", "max_us"} of what was recorded (None if nothing was)."""
        if every > 0:
            self.allreduce_timing = {"every": int(every), "events": []}
            return None
        timing, self.allreduce_timing = self.allreduce_timing, None
        if not timing or not timing["events"]:
            return None
        torch.cuda.synchronize(self.W.device)
        us = [a.elapsed_time(b) * 1e3 for a, b in timing["events"]]
        return {"samples": len(us), "mean_us": sum(us) / len(us), "max_us": max(us)}

    # ------------------------------------------------------------------ checkpoint / resume
    _STATE_FIELDS = EnvState.FIELDS

    def state_dict(self) -> dict:
        """Everything a bit-identical continuation needs: the env SoA, W, the classifier table, the option graph, the
        enabled mask, the step counter (RNG streams are keyed by (seed, global env id, t): no RNG state to save) and,
        when tracing, the trajectory ring + events + the examples collected so far. Tensors are copied to the host."""
        d = {"format": 1, "n_envs": self.n_envs, "n_options": self.n_options, "t": int(self.t),
             "enabled_mask": int(self.enabled_mask), "parents": torch.as_tensor(self.ctx.parents.copy()),
             "W": self.W.cpu(), "clf": self.clf.cpu(),
             "state": {f: getattr(self.state, f).cpu() for f in self._STATE_FIELDS}}
        if self.trace is not None:
            ring_x, ring_y, events, ev_len = self.trace
            d["trace"] = {"ring_x": ring_x.cpu(), "ring_y": ring_y.cpu(), "events": events.cpu(), "ev_len": ev_len.cpu()}
            d["ex_cap"] = self._ex_cap
            d["examples"] = {int(k): (xy[: int(cnt.item())].cpu(), lab[: int(cnt.item())].cpu())
                             for k, (xy, lab, cnt, _) in self._ex.items()}
            d["prev_in"] = {int(k): v[3].cpu() for k, v in self._ex.items() if v[3] is not None}
        d["gest_mask"] = int(self.gest_mask)
        d["gest_need"] = {int(k): int(v) for k, v in self._gest_need.items()}
        if self.gest_mask:
            d["gest_succ"] = self.ctx.set_gestation(self.gest_mask).cpu()
        return d

    def load_state_dict(self, d: dict) -> None:
        if d.get("format") != 1 or d["n_envs"] != self.n_envs or d["n_options"] != self.n_options:
            raise ValueError("checkpoint does not match this agent (format / n_envs / n_options)")
        self.W.copy_(d["W"]); self.clf.copy_(d["clf"])
        for f in self._STATE_FIELDS:
            getattr(self.state, f).copy_(d["state"][f])
        self.t, self.enabled_mask = int(d["t"]), int(d["enabled_mask"])
        if self.n_options:
            self.ctx.set_option_parents([int(v) for v in d["parents"]])
        if "trace" in d:
            self.enable_tracing(int(d["trace"]["ring_x"].shape[0]), int(d["ex_cap"]))
            for name, buf in zip(("ring_x", "ring_y", "events", "ev_len"), self.trace):
                buf.copy_(d["trace"][name])
            for k, (xy, lab) in d["examples"].items():
                bxy, blab, cnt, prev = self._ex_buffers(int(k))
                bxy[: xy.shape[0]].copy_(xy); blab[: lab.shape[0]].copy_(lab); cnt.fill_(int(lab.shape[0]))
                if prev is not None and int(k) in d["prev_in"]:
                    prev.copy_(d["prev_in"][int(k)])
        self.gest_mask = int(d.get("gest_mask", 0))
        self._gest_need = {int(k): int(v) for k, v in d.get("gest_need", {}).items()}
        if self.gest_mask:
            self.ctx.set_gestation(self.gest_mask).copy_(d["gest_succ"])
        self.ctx.invalidate_order()      # option ids were written outside scg_step: the next step sorts afresh (same order)

    def save(self, path: str) -> None:
        torch.save(self.state_dict(), path)

    def load(self, path: str) -> None:
        self.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))

    def q_update(self, k: int, s, action, r, cont, s_next, apply: bool = True) -> None:
        """Batched intra-option Q-learning update of VF k on explicit transitions (SPEC §5):
        delta = r + cont * max_a' Q_k(s',a') - Q_k(s,a);  W_k[a] += alpha/n * scale * sum delta*phi(s)."""
        self.ctx.q_update(k, s, action, r, cont, s_next, self.W, apply=apply)

    def evaluate(self, n_episodes: int = 4096, epsilon: float = 0.0, seed: Optional[int] = None, steps_per_launch: int = 64,
                 per_env: bool = False, states=None, interrupt: bool = False, choose: Optional[str] = None,
                 discounted: bool = False, gate="agent"):
        """How good the current policy is: one episode per env on `n_episodes` envs of a separate evaluation context (cached per
        n_episodes; another seed replaces the entry), acting with `epsilon` and the current W, clf and enabled options, weights
        frozen (SPEC §8). Returns
        EpisodeStats.summary(): episodes, success_rate, mean_return, mean_length and per value function steps_share, entries,
        declines, successes; with per_env=True also the per-env counter tensors, as (summary, dict).
        One BEGIN | ONE_EPISODE launch, then ONE_EPISODE launches up to ceil(max_episode_steps / steps_per_launch) in all: every
        episode has ended by then (time limit), and nothing is read back before the end. The training run is left alone: W,
        state, t, the training context's env order, trace ring, gestation counts and peer exchange counter are untouched.
        A sharded agent evaluates its own rank's policy copy on this rank only: there is no collective here.
        With `states` ((x, y) or (x, y, vx, vy); velocities default to zero) episode i starts from state i instead of a drawn
        start state (SPEC §10's BEGIN_AT), and n_episodes is the number of states.
        With `interrupt` a running option is cut short wherever the root's value at the next state is higher (SPEC §11's
        interrupting rollout); the summary then also holds interrupts per value function.
        With `choose="value"` an env is offered the candidate option whose value at the next state is highest instead of the
        lowest-numbered one (SPEC §14; ValueError for any other value); the summary then also holds overrides per option: the
        entries of an option that was not the lowest-numbered candidate. It combines with `interrupt`.
        With `discounted` the launches also keep each episode's discounted task return (SPEC §15's audited rollout, nothing
        forced): the summary then holds mean_discounted_return and the per-env dict disc_final. No other result changes.
        `gate` (SPEC §25.3): a gate table [n_vf, 2, 5, 1296] (gatefit) under which the value gate compares, None for SPEC §4.2's own
        comparison, default the agent's `gate` (None unless improve_gate(apply=True) stored one). With a table the launches are
        population rollouts of ONE policy (scg_rollout_population_gate), whose range is the plain rollout's by bits but for the
        gate's decisions; ScgError with `interrupt` or `choose`."""
        gate = self._gate_tables(gate, 1)
        pop = None
        if gate is not None:
            dev = self.W.device
            pop = (self.W.reshape(1, self.n_vf, NUM_ACTIONS, NUM_FEATURES), torch.tensor([float(epsilon)], dtype=torch.float32, device=dev),
                   torch.tensor([int(self.enabled_mask)], dtype=torch.int32, device=dev), None, gate)
        stats, _ = self._eval_launches(n_episodes, epsilon, seed, steps_per_launch, states, interrupt, choose=choose,
                                       audit=True if discounted else None, population=pop)
        out = stats.summary()
        return (out, stats.per_env()) if per_env else out

    def record_episodes(self, n_episodes: int = 256, states=None, epsilon: float = 0.0, seed: Optional[int] = None,
                        steps_per_launch: int = 64, interrupt: bool = False, choose: Optional[str] = None, device: bool = False):
        """evaluate() with every step recorded (SPEC §10): the same launches on the same evaluation context, each with a record
        of all envs that is appended to a Trajectory after the launch. Returns (Trajectory, the EpisodeStats summary, equal to
        evaluate()'s with the same arguments). Row 0 of each env is its begin row. The training run is left alone.
        `interrupt`: as for evaluate(); an interrupted step's row has term INTERRUPTED (SPEC §11). `choose`: as for evaluate().
        `device` (SPEC §30.1): the same launches, each appended to a trajectory.DeviceRecord by one scg_record_append call instead:
        nothing is downloaded. Returns (DeviceRecord, the same summary); its to_numpy() is the Trajectory's by bits."""
        stats, traj = self._eval_launches(n_episodes, epsilon, seed, steps_per_launch, states, interrupt, record=True, choose=choose,
                                          device=device)
        return traj, stats.summary()

    def _eval_launches(self, n_episodes, epsilon, seed, steps_per_launch, states, interrupt, record: bool = False, choose=None,
                       audit=None, population=None, W=None, device: bool = False):
        """The launches of evaluate() / record_episodes() on the evaluation context for this episode count and seed, its settings
        copied from training (epsilon aside), stats zeroed and, with `states`, the start states written into its env state: the
        first begins every episode at t0 = 0, launch i > 0 goes on at t0 = 1 + i * steps_per_launch. Returns (EpisodeStats, Trajectory or None).
        `audit` (True: a new GateAudit without a force; or a force vector, one int8 per episode) makes every launch an audited one
        (SPEC §15); the force acts in the first launch, and the GateAudit is left in stats.audit.
        `population` = (W [C, n_vf, 5, 1296], epsilon [C] or None, enabled [C] or None) on the device makes every launch a
        population rollout (SPEC §21) of C policies over n_episodes envs each: the context has C * n_episodes envs, the `states`
        are repeated for every policy, and `epsilon` is the context's own (no policy's, where the population gives one). A fourth
        element, a [C, n_vf, 8] classifier table (or None), gives every policy its own classifiers (SPEC §24.1), a fifth, a
        [C, n_vf, 2, 5, 1296] gate table (or None), its own value gate (SPEC §25.1).
        `W`: the value tables the launches act under instead of the agent's (SPEC §30.3: a record under a table that is not the
        agent's; self.W is not written). `device` with `record`: the launches' rows go to a DeviceRecord (SPEC §30.1), which is
        returned in the Trajectory's place; the Trajectory then serves as the launch buffers only."""
        if choose not in (None, "value"):
            raise ValueError(f"choose must be None or 'value', not {choose!r}")
        if states is not None:
            states = self._start_states(states, 0, 0)
            n_episodes = states[0].numel()
        n, spl = int(n_episodes), int(steps_per_launch)
        if n < 1:
            raise ValueError("n_episodes must be >= 1")
        if not (1 <= spl <= _lib.ROLLOUT_MAX_STEPS):
            raise ValueError(f"steps_per_launch must be in [1, {_lib.ROLLOUT_MAX_STEPS}]")
        c = self.ctx.cfg
        W, kw = (self.W if W is None else W), {}
        if population is not None:
            W, pol_eps, pol_enabled, *pol_clf = population
            n_pol = int(W.shape[0])
            if n * n_pol > 2 ** 31 - 1:
                raise ValueError(f"{n_pol} policies x {n} episodes are more envs than a context holds")
            if states is not None:
                states = [s.repeat(n_pol) for s in states]
            n, kw["population"] = n * n_pol, (pol_eps, pol_enabled, *pol_clf)
        ectx, st, stats = self._eval_context(n, epsilon, seed, states)
        traj = Trajectory(n, spl + 1, 0, ectx.device, n_vf=self.n_vf) if record else None
        rec = DeviceRecord(ectx, n, int(c.max_episode_steps) + 1, n_vf=self.n_vf) if record and device else None
        if audit is not None:
            stats.audit = GateAudit(n, ectx.device, force=None if audit is True else audit)
            kw["audit"] = stats.audit
        for i in range(-(-int(c.max_episode_steps) // spl)):
            ectx.rollout(st, W, self.clf, self.enabled_mask, 0 if i == 0 else 1 + i * spl, spl, stats,
                         begin=(i == 0 and states is None), one_episode=True, begin_at=(i == 0 and states is not None),
                         record=traj, interrupt=interrupt, choose=choose, **kw)
            if audit is not None:
                stats.audit.force = None                       # the force is the begin pseudo-step's alone
            if rec is not None:
                rec.append(traj)
            elif record:
                traj.append()
        return stats, (traj if rec is None else rec)

    def evaluate_policies(self, W, epsilons=None, enabled=None, n_episodes: int = 4096, seed: Optional[int] = None,
                          steps_per_launch: int = 64, states=None, interrupt: bool = False, choose: Optional[str] = None,
                          per_env: bool = False, baseline: int = 0, clf=None, gate="agent"):
        """Several policies in one set of launches, on common random numbers (SPEC §21): `W` is [C, n_vf, 5, 1296] or a list of C
        [n_vf, 5, 1296] tables, `epsilons` and `enabled` scalars or one per policy (defaults: 0.0 and the agent's enabled mask).
        evaluate(discounted=True)'s launches run ONCE, on an evaluation context of C * n_episodes envs of which the envs c *
        n_episodes .. (c + 1) * n_episodes - 1 act under policy c; env i of every policy sees the same start state (`states`, as for
        evaluate(), are repeated for every policy) and the same draws. Returns (summaries, paired): summaries[c] is what
        evaluate(n_episodes, epsilon=epsilons[c], discounted=True, ...) returns with W[c] and enabled[c] in place, field for field;
        paired[c] is evaluation.paired_differences of policy c against policy `baseline` (exact zeros for the baseline itself and
        for any policy equal to it). With per_env=True also the list of the policies' per-env dicts, as (summaries, paired,
        per_envs). The training run is left alone exactly as by evaluate(). ValueError for C outside 1 .. 64, for more than 2^31 - 1
        envs in all, and for `epsilons` / `enabled` of another length.
        `clf` (SPEC §24.3): None (the agent's classifier table for every policy), one [n_vf, 8] table for all of them, or [C, n_vf, 8]
        / a list of C tables, one per policy: summaries[c] is then evaluate()'s with clf[c] in place too. With `clf` given, `W` may
        also be a single [n_vf, 5, 1296] table, repeated for every policy of clf (comparing classifiers under one W).
        `gate` (SPEC §25.3): None (SPEC §4.2's comparison for every policy), one [n_vf, 2, 5, 1296] gate table for all of them, or
        [C, n_vf, 2, 5, 1296] / a list of C tables, one per policy; default the agent's `gate`. summaries[c] is then evaluate()'s
        with gate[c] too. With C tables given, `W` may be a single table as with `clf`. ScgError with `interrupt` or `choose`."""
        dev = self.W.device
        table = (self.n_vf, NUM_ACTIONS, NUM_FEATURES)
        row = (self.n_vf, _lib.CLF_STRIDE)
        gate = self._gate_tables(gate, None)
        if gate is not None and clf is None and not isinstance(W, (list, tuple)):
            W = torch.as_tensor(W, dtype=torch.float32).to(dev)
            if W.dim() != 4 and W.numel() == self.W.numel():           # one W for every policy of gate
                W = W.reshape(1, *table).repeat(int(gate.shape[0]), 1, 1, 1)
        if clf is not None:
            if isinstance(clf, (list, tuple)):
                clf = [torch.as_tensor(t, dtype=torch.float32).to(dev) for t in clf]
                if not clf or any(tuple(t.shape) != row for t in clf):
                    raise ValueError(f"every table of clf must be {list(row)}")
                clf = torch.stack(clf)
            clf = torch.as_tensor(clf, dtype=torch.float32).to(dev)
            if clf.dim() not in (2, 3) or tuple(clf.shape[-2:]) != row:
                raise ValueError(f"clf must be {list(row)} or [C, {row[0]}, {row[1]}], not {tuple(clf.shape)}")
            if not isinstance(W, (list, tuple)):
                W = torch.as_tensor(W, dtype=torch.float32).to(dev)
                if W.dim() != 4 and W.numel() == self.W.numel():       # one W for every policy of clf
                    W = W.reshape(1, *table).repeat(int(clf.shape[0]) if clf.dim() == 3 else 1, 1, 1, 1)
        if isinstance(W, (list, tuple)):
            W = [torch.as_tensor(w, dtype=torch.float32).to(dev) for w in W]
            if not W or any(w.numel() != self.W.numel() for w in W):
                raise ValueError(f"every table of W must be {list(table)}")
            W = torch.stack([w.reshape(table) for w in W])
        W = torch.as_tensor(W, dtype=torch.float32).to(dev)
        if W.dim() != 4 or tuple(W.shape[1:]) != table:
            raise ValueError(f"W must be [C, {self.n_vf}, {NUM_ACTIONS}, {NUM_FEATURES}], not {tuple(W.shape)}")
        n_pol = int(W.shape[0])
        if not (1 <= n_pol <= _lib.POP_MAX):
            raise ValueError(f"evaluate_policies takes 1 .. {_lib.POP_MAX} policies, not {n_pol}")
        if not (0 <= int(baseline) < n_pol):
            raise ValueError(f"baseline must name a policy 0 .. {n_pol - 1}")

        def per_policy(v, default, dtype, what):
            v = np.asarray(default if v is None else v)
            if v.ndim == 0:
                v = np.full(n_pol, v)
            if v.shape != (n_pol,):
                raise ValueError(f"{what} must be a scalar or hold one entry per policy ({n_pol}), not {v.shape}")
            return torch.from_numpy(np.ascontiguousarray(v.astype(dtype))).to(dev)

        pol_eps = per_policy(epsilons, 0.0, np.float32, "epsilons")
        pol_enabled = per_policy(enabled, self.enabled_mask, np.int32, "enabled")
        pol_clf = ()
        if clf is not None:
            if clf.dim() == 2:
                clf = clf.reshape(1, *row).repeat(n_pol, 1, 1)
            if int(clf.shape[0]) != n_pol:
                raise ValueError(f"clf must hold one table per policy ({n_pol}), not {int(clf.shape[0])}")
            pol_clf = (clf.contiguous(),)
        if gate is not None:
            if int(gate.shape[0]) == 1:
                gate = gate.repeat(n_pol, 1, 1, 1, 1)
            if int(gate.shape[0]) != n_pol:
                raise ValueError(f"gate must hold one table per policy ({n_pol}), not {int(gate.shape[0])}")
            pol_clf = (pol_clf[0] if pol_clf else None, gate.contiguous())
        # (the context's own epsilon is read by no policy: every one has its entry; with clf the agent's table likewise)
        stats, _ = self._eval_launches(n_episodes, 0.0, seed, steps_per_launch, states, interrupt, choose=choose, audit=True,
                                       population=(W.contiguous(), pol_eps, pol_enabled, *pol_clf))
        n = stats.n // n_pol
        summaries = [stats.summary(c * n, (c + 1) * n) for c in range(n_pol)]
        envs = [{f: v.detach().cpu() for f, v in stats.per_env(c * n, (c + 1) * n).items()} for c in range(n_pol)]
        paired = [paired_differences(envs[c], envs[int(baseline)]) for c in range(n_pol)]
        return (summaries, paired, envs) if per_env else (summaries, paired)

    def _gate_tables(self, gate, n_pol: Optional[int]):
        """`gate` of evaluate() / evaluate_policies() as a float32 [C, n_vf, 2, 5, 1296] device tensor, or None: "agent" is the
        agent's own; one table is C = 1; a list is stacked. n_pol = 1 takes one table only."""
        if isinstance(gate, str):
            if gate != "agent":
                raise ValueError(f"gate must be a table, None or 'agent', not {gate!r}")
            gate = getattr(self, "gate", None)                 # (a stand-in agent without the attribute: no table)
        if gate is None:
            return None
        shape = (self.n_vf, 2, NUM_ACTIONS, NUM_FEATURES)
        if isinstance(gate, (list, tuple)):
            gate = [torch.as_tensor(t, dtype=torch.float32).to(self.W.device) for t in gate]
            if not gate or any(tuple(t.shape) != shape for t in gate):
                raise ValueError(f"every table of gate must be {list(shape)}")
            gate = torch.stack(gate)
        gate = torch.as_tensor(gate, dtype=torch.float32).to(self.W.device)
        if gate.dim() == 4:
            gate = gate[None]
        if gate.dim() != 5 or tuple(gate.shape[1:]) != shape or (n_pol is not None and int(gate.shape[0]) != n_pol):
            raise ValueError(f"gate must be {list(shape)}" + (" or [C, ...] / a list of such tables" if n_pol is None else "")
                             + f", not {tuple(gate.shape)}")
        return gate.contiguous()

    def improve_policy(self, lambdas=(0.25, 0.5, 1.0), eval_epsilons=(0.0,), criterion: str = "discounted", z: float = 2.0,
                       n_eval: int = 4096, apply: bool = False, **fit):
        """A safeguarded policy-improvement step (SPEC §21.4): fit_values_to_branches(apply=False, **fit) gives W_new; the
        candidates W and valuefit.damped_tables(W, W_new, lambdas) at each of `eval_epsilons` are evaluated in ONE
        evaluate_policies run of n_eval episodes each (common random numbers; the baseline of a candidate is W at the same
        epsilon); the decision is taken at eval_epsilons[0] by valuefit.choose_candidate: the candidate with the highest mean of `criterion`,
        ties to the smallest lambda, accepted only where its paired mean difference against W exceeds z standard errors (z = 2:
        §19.4's "beyond two standard errors" convention, a parameter). Returns (report, W_chosen): report["fit"] the fit's
        report, report["candidates"] rows of {"lambda", "epsilon", "summary", "paired"} (lambda = 0: W itself), "chosen_lambda" (0.0
        when W is kept), "accepted", "criterion", "z"; W_chosen a copy of the chosen table (of W when kept). apply=True copies
        W_chosen into W when accepted. Refusals: fit_values_to_branches's; ValueError for no lambda, a lambda of 0, no epsilon or
        an unknown criterion. With apply=False the agent is left as evaluate() leaves it."""
        from .valuefit import choose_candidate, damped_tables
        lam = [float(v) for v in lambdas]
        eps = [float(v) for v in eval_epsilons]
        if not lam or not eps or any(v == 0.0 for v in lam):
            raise ValueError("improve_policy needs at least one lambda, none of them 0, and at least one epsilon")
        if criterion not in ("discounted", "return", "success"):
            raise ValueError(f"criterion must be 'discounted', 'return' or 'success', not {criterion!r}")
        if apply and self.group is not None:
            raise ScgError("improve_policy(apply=True) with shared weights: each rank would choose its own table and the ranks would part")
        fit_report, W_new = self.fit_values_to_branches(apply=False, **fit)
        shape = (self.n_vf, NUM_ACTIONS, -1)
        tables = torch.cat([self.W.reshape(1, *shape), damped_tables(self.W.reshape(shape), W_new.reshape(shape), lam)])
        lam0, n_tab = [0.0] + lam, 1 + len(lam)
        per_eps = len(eps)
        # policy e * n_tab + i: table i at epsilon e; its baseline W at that epsilon is policy e * n_tab. One run per baseline would
        # pair against one policy only, so the paired rows are taken here from the per-env dicts of the single run.
        summaries, _, envs = self.evaluate_policies(tables.repeat(per_eps, 1, 1, 1), np.repeat(np.asarray(eps, np.float32), n_tab),
                                                    None, n_episodes=int(n_eval), seed=fit.get("seed"),
                                                    interrupt=bool(fit.get("interrupt", False)), choose=fit.get("choose"), per_env=True)
        rows = [{"lambda": lam0[i], "epsilon": eps[e], "summary": summaries[e * n_tab + i],
                 "paired": paired_differences(envs[e * n_tab + i], envs[e * n_tab])} for e in range(per_eps) for i in range(n_tab)]
        pick = choose_candidate(rows[:n_tab], criterion, z)
        W_chosen = (tables[pick["index"]] if pick["accepted"] else tables[0]).reshape(self.W.shape).clone()
        if apply and pick["accepted"]:
            self.W.copy_(W_chosen)
        return {"fit": fit_report, "candidates": rows, "chosen_lambda": pick["chosen_lambda"], "accepted": pick["accepted"],
                "criterion": criterion, "z": float(z)}, W_chosen

    def _eval_context(self, n: int, epsilon: float, seed: Optional[int], states):
        """The evaluation context for `n` episodes and `seed` (None: training's), its settings copied from training (epsilon
        aside), its stats zeroed and, with `states`, the start states written into its env state: (context, EnvState, EpisodeStats)."""
        seed = int(self.ctx.cfg.seed) if seed is None else int(seed)
        # one evaluation context per n_episodes; the seed is a create-time setting, so another seed replaces that entry (a
        # caller sweeping seeds holds one context, not one per seed)
        cache = self._eval_ctx
        if n not in cache or cache[n][0].cfg.seed != seed:
            if n in cache:
                cache.pop(n)[0].close()
            ectx = ScgContext(n, self.n_options, self.map, device=self.ctx.device.index, seed=seed, env_id_base=0,
                              block_envs=self.ctx.block_envs)
            cache[n] = (ectx, EnvState(n, ectx.device, self.map), EpisodeStats(self.n_vf, n, ectx.device))
        ectx, st, stats = cache[n]
        self._mirror_training(ectx, epsilon)
        stats.zero_()
        if states is not None:
            for dst, src in zip((st.x, st.y, st.vx, st.vy), states):
                dst.copy_(src.to(dst.device))
        return ectx, st, stats

    def gate_audit(self, k: Optional[int] = None, states=None, n_states: int = 4096, epsilon: float = 0.0,
                   seed: Optional[int] = None, interrupt: bool = False, choose: Optional[str] = None) -> dict:
        """Does the value gate decide right (SPEC §15)? From every start state (`states` as for evaluate(); default: n_states
        map.sample_free positions at rest) two episodes are run on the evaluation context, one FORCED to enter option k at the
        start and one forced to decline it, with the same seed and step counters, so the same random numbers afterwards; with
        epsilon = 0 the pair is deterministic. `k = None`: each state's own lowest-numbered candidate. States where k is no
        candidate are left out. Returns GateAudit.pair_summary()'s dict ("overall", "options") plus "per_state": the kept
        states' index, option, v_k, v_0, g_enter, g_decline, goal_enter, goal_decline (host arrays, state order). W, the
        training state and t are untouched. `interrupt`, `choose`: the rules of every later step, as for evaluate()."""
        if k is not None and not (1 <= int(k) <= self.n_options):
            raise ValueError(f"k must be None or an option 1..{self.n_options}")
        states = self._start_states(states, n_states, 0 if seed is None else int(seed))
        n = states[0].numel()
        run = lambda force, **kw: self._eval_launches(n, epsilon, seed, 64, states, interrupt, choose=choose, audit=force, **kw)[0]
        if k is None:                                          # min C of each state: the option an unforced begin offers (§4.2)
            ectx, st, _ = self._eval_context(n, epsilon, seed, states)
            probe = GateAudit(n, ectx.device)
            ectx.rollout(st, self.W, self.clf, self.enabled_mask, 0, 0, None, begin_at=True, audit=probe)      # a 0-step begin launch
            ks = probe.cand
        else:
            ks = torch.full((n,), int(k), dtype=torch.int8, device=self.W.device)
        res = []
        for sign in (1, -1):
            stats = run(sign * ks)
            res.append(dict(stats.audit.host(), goals=stats.goals.cpu().numpy().copy()))
        ent, dec = res
        keep = (ent["applied"] == 1) & (dec["applied"] == 1)
        per = {"index": np.nonzero(keep)[0], "option": ent["cand"][keep].astype(np.int64),
               "v_k": ent["v_cand"][keep], "v_0": ent["v_root"][keep],
               "g_enter": ent["disc_final"][keep], "g_decline": dec["disc_final"][keep],
               "goal_enter": ent["goals"][keep] > 0, "goal_decline": dec["goals"][keep] > 0}
        out = GateAudit.pair_summary(per["option"], per["v_k"], per["v_0"], per["g_enter"], per["g_decline"],
                                     per["goal_enter"], per["goal_decline"])
        out["per_state"] = per
        return out

    def fit_values_to_returns(self, n_episodes: int = 4096, epsilon: float = 0.1, seed: Optional[int] = None, vfs=None,
                              ridge: float = 1e-3, apply: bool = False, interrupt: bool = False, choose: Optional[str] = None,
                              keep: bool = False, order: Optional[int] = None, trajectory=None, lam=None, sweeps: int = 1, trace: str = "peng",
                              double: bool = False, pipeline: str = "host", fresh: bool = False, solver: str = "host"):
        """The best linear fit of each Q_k to the returns its own policy realises (SPEC §16, §18, §27 - §31): one loop over a flat view
        of a record (valuefit.flat_view / DeviceRecord.flat: the rows in (env, row) order on the device, with their row tables).
        The record is record_episodes() with the current policy, or `trajectory`, a kept record (report["trajectory"] of an earlier
        call; report["episodes"] is then None). Every sweep forms its targets y over all rows and then, per value function k of `vfs`
        (default: all), runs one unit (_fit_unit): the sample list — the step rows with vf = k of the EVEN envs sorted by action with
        a stable sort, then those of the odd envs, which are held out; a sample's state is that of the row before —, Q^old of the
        samples, the residual d = float32(y - float64 Q^old), per action A, b by ScgContext.feature_gram with the action as segment,
        Delta by valuefit.ridge_solve on the host, W_k[a] <- float32(W_k^old[a] + Delta) (an action without samples keeps its row bit
        for bit), and Q^new. Returns (report, W_new): W_new a copy of W with the fitted rows; report["vf"][k] holds n (fit samples per
        action), delta_norm and, for "fit" and "held_out", old / new: n, rmse, mean_error of Q^old / Q^new against y. The held-out
        numbers are the ones that count. `keep` adds report["vf"][k]["operands"] (states, action, y, d, offsets, n_fit, A, b, rows,
        delta), report["targets"] (returns_to_go's dict) and report["trajectory"].
        apply=False leaves the agent as evaluate() does: W, training state, t, env order, trace ring, gestation counts and peer
        counter untouched. apply=True copies the fitted rows of `vfs` into W; refused with shared weights (a sharded agent would
        fit its own rank's copy only, and the ranks' W would part).
        The targets. lam=None: the Monte-Carlo targets of valuefit.returns_to_go, one sweep. `lam` in [0, 1] (SPEC §27): the
        lambda-returns of valuefit.sweep_targets under the table the sweep starts from (lam = 1: the Monte-Carlo return, lam = 0:
        §17.2's one-step target); `sweeps` = S re-forms them under the sweep before's W_new on the same record and refits from it
        (fitted policy evaluation). The report adds "lam", "trace" and "sweeps" (per sweep "vf" and "W"; report["vf"] is the last
        sweep's), per value function "mc" (the error block against the MONTE-CARLO targets, so that every lam is judged on §16's
        scale) and with `keep` report["lambda_targets"] (valuefit.lambda_targets' / trace_targets' dict of the last sweep).
        `trace` (SPEC §28): "watkins" cuts the trace wherever the recorded action is not the greedy action of the table bootstrapped
        from, so the targets evaluate that table's greedy policy; `lam` may be a sequence of n_vf floats, one per value function,
        with either trace. Both take the targets from ScgContext.trace_returns ("peng" with a float: lambda_returns) and add
        valuefit.trace_stats' "cut_share", "off_greedy", "horizon" and "a_changed" (None in the first sweep) per value function.
        `order` = p in (3, 5, 7) (SPEC §18's basis-order probe, Monte-Carlo targets only): the residual is regressed on the (p + 1)^4
        features of order p (ScgContext.basis_gram, Lambda from order p's scale table, the solve on the device) while Q^old stays the
        agent's order-5 value: Q^new = float32(Q^old + v), v = ScgContext.basis_values(float32(Delta))[a], the sum in float64. The
        report adds "order", "features" and per value function "delta" (float64 [5][F]); W_new is a plain copy of W.
        `double` (SPEC §29.2; needs lam): every sweep is _double_sweep — two tables on two folds of the fit half, each bootstrapping
        from the other's value of its own greedy action, one unit per fold; W_new is their mean, which the held-out half judges.
        `pipeline`: where the view comes from and how Q of a sample list is formed. "host": the Trajectory uploaded once per call,
        ScgContext.q_values in chunks of the evaluation context's n_envs. "device" (SPEC §30.2; needs lam): a trajectory.DeviceRecord
        (recorded with device=True; a Trajectory given as `trajectory` is uploaded into one), one ScgContext.row_action_values call,
        as under `double`; report["trajectory"] is the DeviceRecord. W_new and every reported number are equal.
        `fresh` (SPEC §30.3; needs lam, implies pipeline="device"): every sweep s after the first records `n_episodes` new episodes
        under the table the sweep before handed on, with this call's epsilon, interrupt and choose and the seed `seed` + s - 1, and
        takes its targets, samples and held-out half from that record. Every sweep's entry then holds "episodes" (its record's
        summary), its "mc" is against its own record's returns, and "a_changed" is None: the rows differ between sweeps.
        `solver` (SPEC §31.3): who solves the refit's normal equations. "host": valuefit.ridge_solve on the downloaded Gram (with
        `order` its device form, a vendor Cholesky per action). "device": valuefit.ridge_solve_pinned in every mode — both pipelines,
        `double`, `fresh` and `order` —: A and b stay where the Gram call left them, the new rows are formed on the device by the same
        two roundings, and only `info` and the 5 x F Delta of the report come back. Its W_new has the bits of a host model of SPEC
        §31.1's order, not LAPACK's: the two solvers' tables differ in the last places.
        Refused (ScgError): a trace other than the two names; a solver other than the two names; "watkins", double,
        pipeline="device" or fresh without lam; double,
        pipeline="device", fresh or lam with order; pipeline="device" or fresh with double; a lam outside [0, 1] or a lam sequence of
        another length than n_vf; sweeps < 1, or != 1 without lam; order with apply=True; apply=True with shared weights."""
        from .core import fourier_scale_table
        from .valuefit import flat_view, host_targets, returns_to_go, sweep_targets, trace_stats
        if trace not in ("peng", "watkins"):
            raise ScgError(f"fit_values_to_returns: trace must be 'peng' or 'watkins', not {trace!r}")
        if solver not in ("host", "device"):
            raise ScgError(f"fit_values_to_returns: solver must be 'host' or 'device', not {solver!r}")
        if trace == "watkins" and lam is None:
            raise ScgError("fit_values_to_returns: trace='watkins' needs lam (the Monte-Carlo path has no trace to cut)")
        if double and (lam is None or order is not None):
            raise ScgError("fit_values_to_returns: double=True needs lam (the Monte-Carlo targets bootstrap from nothing) and "
                           "cannot be given with order")
        if pipeline not in ("host", "device"):
            raise ScgError(f"fit_values_to_returns: pipeline must be 'host' or 'device', not {pipeline!r}")
        if fresh and (lam is None or double or order is not None):
            raise ScgError("fit_values_to_returns: fresh=True needs lam and cannot be given with double or order")
        if fresh:
            pipeline = "device"
        if pipeline == "device" and lam is None:
            raise ScgError("fit_values_to_returns: pipeline='device' needs lam (the Monte-Carlo path stays on the host)")
        if pipeline == "device" and order is not None:
            raise ScgError("fit_values_to_returns: pipeline='device' cannot be given with order")
        if pipeline == "device" and double:
            raise ScgError("fit_values_to_returns: pipeline='device' cannot be given with double=True")
        lam_seq = lam is not None and np.ndim(lam) != 0
        if lam is not None:
            if order is not None:
                raise ScgError("fit_values_to_returns: lam and order cannot be given together (the lambda-return bootstraps from the "
                               "order-5 tables)")
            if lam_seq:
                lam = [float(v) for v in lam]
                if len(lam) != self.n_vf or not all(0.0 <= v <= 1.0 for v in lam):
                    raise ScgError(f"fit_values_to_returns: a lam sequence must hold {self.n_vf} values in [0, 1], one per value function")
            elif not (0.0 <= float(lam) <= 1.0):
                raise ScgError("fit_values_to_returns: lam must be None or lie in [0, 1]")
        traced = trace == "watkins" or lam_seq                 # SPEC §28: the targets come from trace_targets
        if int(sweeps) < 1 or (lam is None and int(sweeps) != 1):
            raise ScgError("fit_values_to_returns: sweeps must be >= 1, and 1 without lam")
        if order is not None:
            if order not in _lib.BASIS_ORDERS:
                raise ScgError(f"fit_values_to_returns: order must be None or one of {_lib.BASIS_ORDERS}")
            if apply:
                raise ScgError(f"fit_values_to_returns(order={order}, apply=True): the fit at a basis order is a report; no kernel acts "
                               f"on weights of {_lib.basis_features(order)} features")
        if apply and self.group is not None:
            raise ScgError("fit_values_to_returns(apply=True) with shared weights: each rank would fit its own copy of W and the "
                           "ranks would part; fit with apply=False and load one rank's result on all of them")
        vfs = list(range(self.n_vf)) if vfs is None else [int(k) for k in vfs]
        if any(not (0 <= k < self.n_vf) for k in vfs):
            raise ValueError(f"vfs must name value functions 0..{self.n_vf - 1}")
        c = self.ctx.cfg
        gamma, r_succ = float(c.gamma), float(c.r_option_success)
        seed0 = int(c.seed) if seed is None else int(seed)
        device = pipeline == "device"
        if isinstance(trajectory, DeviceRecord) and not device:
            trajectory = trajectory.to_trajectory()
        if trajectory is None:
            rec, summary = self.record_episodes(n_episodes, epsilon=epsilon, seed=seed, interrupt=interrupt, choose=choose, device=device)
            ectx = self._eval_ctx[int(n_episodes)][0]
        else:
            rec, summary = trajectory, None
            ectx = self._eval_context(int(rec.n), epsilon, seed, None)[0]
            if device and not isinstance(rec, DeviceRecord):
                rec = DeviceRecord.from_trajectory(ectx, rec)
        report = {"episodes": summary, "ridge": float(ridge), "vf": {}}
        if order is not None:
            report["order"], report["features"] = int(order), _lib.basis_features(order)
        if lam is not None:
            report["lam"], report["sweeps"], report["trace"] = (list(lam) if lam_seq else float(lam)), [], trace
        # the one difference in the arithmetic's calls: how Q of a sample list is formed
        q_of = self._q_rows if device or double else self._q_chunks
        scale = self.ctx.scale if order is None else fourier_scale_table(order)
        W_new = self.W.clone()
        W_a, W_b = (self.W.clone(), self.W.clone()) if double else (None, None)
        ag_prev = None
        for sweep in range(int(sweeps)):
            if fresh and sweep:                                # SPEC §30.3: sweep s (from 1) records under the table handed on, at seed + s
                ectx, rec, summary = self._record_under(W_new.clone(), n_episodes, epsilon, seed0 + sweep, interrupt, choose)
            if fresh or not sweep:                             # a new record: its flat view, its halves and Monte-Carlo targets
                if device:
                    fl = rec.flat(ectx)
                    if "tabA" not in fl or any(f not in fl for f in ("x", "y", "vx", "vy", "reward", "action")):
                        raise ScgError("fit_values_to_returns: the record must hold the state, reward, action, done, vf and term fields")
                flat = rec.to_numpy()                          # (of a DeviceRecord: ONE download of the record)
                if not device:
                    fl = flat_view(ectx, flat)
                tg = returns_to_go(flat, gamma, r_succ)
                even = fl["env"] % 2 == 0                      # the fit half, by action; the odd envs are held out
                lists = {} if double else {k: (self._sample_rows(fl, k, even, by_action=True), self._sample_rows(fl, k, ~even))
                                           for k in vfs}
                unit = functools.partial(self._fit_unit, ectx, fl, None if lam is None else tg["y"], q_of, ridge, order, scale,
                                         solver=solver)
            if double:
                report["vf"], W_new, lt = self._double_sweep(unit, ectx, fl, tg["y"], q_of, vfs, W_a, W_b, gamma, lam, r_succ,
                                                             trace == "watkins", keep)
                entry = {"vf": report["vf"], "W": W_new.clone(), "W_a": W_a.clone(), "W_b": W_b.clone()}
            else:
                W_cur = W_new.clone()                          # what the targets bootstrap from and the residual is taken against
                lt = {"y": torch.from_numpy(tg["y"]).to(W_cur.device)} if lam is None else \
                    sweep_targets(ectx, fl, W_cur, gamma, lam, r_succ, traced=traced, cut=trace == "watkins")
                report["vf"] = {}
                for k in vfs:
                    rows = torch.cat(lists[k])
                    rep, operands = unit(k, rows, lists[k][0].numel(), lt["y"], W_cur, W_new)
                    if traced:
                        rep.update(trace_stats(lt, rows, ag_prev))
                    if keep:
                        rep["operands"] = operands
                    report["vf"][k] = rep
                entry = {"vf": report["vf"], "W": W_new.clone()}
                ag_prev = lt["ag"] if traced and not fresh else None
            if fresh:
                entry["episodes"] = summary
            if lam is not None:
                report["sweeps"].append(entry)
        if double:
            report["double"] = {"W_a": W_a, "W_b": W_b}
        if keep:
            report["targets"], report["trajectory"] = tg, rec
            if double:
                report["double_targets"] = {"AB": host_targets(fl, lt["a"]), "BA": host_targets(fl, lt["b"])}
            elif lam is not None:
                report["lambda_targets"] = host_targets(fl, lt)
        if apply:
            for k in vfs:
                self.W[k].copy_(W_new[k])
        return report, W_new

    def _record_under(self, W, n_episodes, epsilon, seed, interrupt, choose):
        """record_episodes(device=True) under the tables W instead of the agent's: (evaluation context, DeviceRecord, summary).
        self.W is not written."""
        stats, rec = self._eval_launches(n_episodes, epsilon, seed, 64, None, interrupt, record=True, choose=choose, W=W, device=True)
        return self._eval_ctx[int(n_episodes)][0], rec, stats.summary()

    def _refit_rows(self, gram, states, d, act_fit, ridge: float, scale, W_k, solver: str = "host", ectx=None):
        """The refit of one table's rows to a residual (SPEC §16.3), the one copy of it: the per-action segments of the fit samples
        (the first len(act_fit) of `states`, sorted by action), A and b by `gram` with yv = d, Delta by valuefit.ridge_solve — on the
        host; with W_k None (the basis-order probe: F up to 4096) on the device, and no row is formed — and W_k[a] <-
        float32(float64 W_k[a] + Delta[a]); an action without samples keeps its row bit for bit. Returns (n_a, offsets, A, b, delta,
        w_new or None). With `solver` "device" (SPEC §31.3) Delta is valuefit.ridge_solve_pinned's under the context `ectx` in either
        case: A and b are not downloaded, the rows are formed on the device by the same two roundings (w_new is then a device
        tensor), and delta is the one 5 x F download."""
        from .valuefit import ridge_solve, ridge_solve_pinned
        dev = self.W.device
        n_a = np.bincount(act_fit, minlength=NUM_ACTIONS).astype(np.int64)
        offsets = np.concatenate([[0], np.cumsum(n_a)]).astype(np.int64)
        A, b = gram(states, offsets, torch.from_numpy(d).to(dev))
        if solver == "device":
            delta_d = ridge_solve_pinned(ectx, A, b, n_a, ridge, scale)
            if W_k is None:
                return n_a, offsets, A, b, delta_d.cpu().numpy(), None
            keep = torch.from_numpy(n_a == 0).to(dev)[:, None]
            w_new = torch.where(keep, W_k, (W_k.double() + delta_d).float())
            return n_a, offsets, A, b, delta_d.cpu().numpy(), w_new
        if W_k is None:
            return n_a, offsets, A, b, ridge_solve(A, b, n_a, ridge, scale, device=dev), None
        delta = ridge_solve(A.cpu().numpy(), b.cpu().numpy(), n_a, ridge, scale)
        w_old = W_k.cpu().numpy()
        w_new = (w_old.astype(np.float64) + delta).astype(np.float32)
        w_new[n_a == 0] = w_old[n_a == 0]
        return n_a, offsets, A, b, delta, w_new

    @staticmethod
    def _sample_rows(fl, k: int, envs, by_action: bool = False):
        """The sample list of value function k in a flat view: the indices of the step rows (row >= 1) with vf = k among the rows
        `envs` marks (a bool tensor over the rows: the envs of a half or a fold), in (env, row) order; with `by_action` sorted by
        action with a stable sort, as the Gram's per-action segments want them. A device int64 tensor."""
        rows = torch.nonzero((fl["row"] >= 1) & (fl["vf"] == int(k)) & envs).view(-1)
        return rows[torch.sort(fl["action"][rows], stable=True)[1]] if by_action else rows

    @staticmethod
    def _q_chunks(ectx, states, W, k: int, act):
        """Q_k(s_n, a_n) of a sample list under the tables W, a float32 host array as the kernel gives it: ScgContext.q_values in
        chunks of the context's n_envs, the host pipeline's way."""
        a = act.cpu().numpy().astype(np.int64)
        out = np.zeros(len(a), np.float32)
        for i in range(0, len(a), ectx.n_envs):
            sl = slice(i, i + ectx.n_envs)
            q = ectx.q_values([t[sl].contiguous() for t in states], W[k].contiguous().view(-1)).cpu().numpy()
            out[sl] = q[a[sl], np.arange(q.shape[1])]
        return out

    @staticmethod
    def _q_rows(ectx, states, W, k: int, act):
        """_q_chunks' array by ONE ScgContext.row_action_values call: the device pipeline's and the double fit's way."""
        tab = torch.full((act.numel(),), int(k), dtype=torch.uint8, device=act.device)
        return ectx.row_action_values(states, tab, W.contiguous().view(-1, NUM_ACTIONS, NUM_FEATURES), act).cpu().numpy()

    def _fit_unit(self, ectx, fl, y_mc, q_of, ridge: float, order, scale, k: int, rows, n_fit: int, y, W_old, W_to, solver: str = "host"):
        """The unit every fit_values_to_returns mode runs per value function (per fold under `double`): table k of W_old refitted on
        the sample list `rows` of the flat view `fl` (a device index tensor; the first n_fit, sorted by action, are fitted, the rest
        held out) to the targets y (a device tensor over all rows). Q^old by `q_of` (_q_chunks or _q_rows) under W_old, the residual
        float32(y - float64 Q^old), _refit_rows, the new row written into W_to[k], Q^new by `q_of` under W_to; with `order` the
        Gram and the solve are order p's, no row is written and Q^new = Q^old + basis_values(Delta). The statistics are
        valuefit.fit_stats on the downloaded per-sample arrays (`y_mc`: the Monte-Carlo targets of all rows, a host array, or None).
        `solver`: _refit_rows'. Returns (the value function's report, its kept operands)."""
        from .valuefit import fit_stats
        dev = self.W.device
        act_d = fl["action"][rows].contiguous()
        act, rows_h, y = act_d.cpu().numpy().astype(np.int64), rows.cpu().numpy(), y[rows].cpu().numpy()
        states = [fl[f][rows - 1].contiguous() for f in ("x", "y", "vx", "vy")]
        q_old = q_of(ectx, states, W_old, k, act_d)
        d = (y - q_old.astype(np.float64)).astype(np.float32)
        if order is None:
            n_a, offsets, A, b, delta, w_new = self._refit_rows(ectx.feature_gram, states, d, act[:n_fit], ridge, scale, W_old[k],
                                                                solver, ectx)
            W_to[k] = w_new if isinstance(w_new, torch.Tensor) else torch.from_numpy(w_new).to(dev)
            q_new = q_of(ectx, states, W_to, k, act_d)
        else:                                                  # (F up to 4096: factored on the device)
            gram = lambda st, offs, yv: ectx.basis_gram(order, st, offs, yv)
            n_a, offsets, A, b, delta, _ = self._refit_rows(gram, states, d, act[:n_fit], ridge, scale, None, solver, ectx)
            q_new = q_old.copy()                               # the correction lives at order p: Q^new = Q^old + Delta . phi^p
            if len(act):
                v = ectx.basis_values(order, states, torch.from_numpy(delta.astype(np.float32)).to(dev)).cpu().numpy()
                q_new = (q_old.astype(np.float64) + v[act, np.arange(len(act))].astype(np.float64)).astype(np.float32)
        rep = {"n": [int(v) for v in n_a], "delta_norm": float(np.sqrt(np.sum(delta * delta)))}
        if order is not None:
            rep["delta"] = delta
        rep.update(fit_stats(q_old, q_new, y, None if y_mc is None else y_mc[rows_h], n_fit))
        return rep, {"states": states, "action": act, "y": y, "d": d, "offsets": offsets, "n_fit": n_fit, "A": A, "b": b,
                     "rows": rows_h, "delta": delta}

    def _double_sweep(self, unit, ectx, fl, y_mc, q_of, vfs, W_a, W_b, gamma: float, lam, r_succ: float, cut: bool, keep: bool):
        """One sweep of fit_values_to_returns(double=True), SPEC §29.2, on the tables W_a and W_b (W to start; refitted in place).
        Two target sets over the whole record by valuefit.sweep_targets — AB: W_a selects the bootstrap action and W_b values it; BA
        the other way round — then `unit` refits table A on fold A's rows (env % 4 == 0: valuefit.fold_of's fold 0) to AB against its
        own Q^old under W_a, and table B on fold B's rows (env % 4 == 2) to BA. W_new = valuefit.mean_table(W_a, W_b); the odd envs
        stay held out and judge the mean table. Returns (the sweep's per-vf report, W_new, {"a": AB, "b": BA}).
        The report has the single fit's layout: per value function n (fit samples per action, both folds), delta_norm (of the mean
        table's row) and valuefit.fit_stats' block of the MEAN table, before and after, against (y_AB + y_BA) / 2 and ("mc") the
        Monte-Carlo targets; "cut_share" / "off_greedy" / "horizon" as the mean of the two target sets' — and adds "folds": {"a",
        "b"}, each n, delta_norm, "fit" and "mc" old / new of the fold's own table on the fold's rows against its own targets
        (`keep`: "operands"), and "optimism": the mean, over the rows whose target reads a bootstrap value of value function k (k = 0:
        tab0's rows, v0; k >= 1: tabk's rows of table k, vk) and both target sets, of vs - v, the selecting table's own maximum less
        the other table's value of that action: the max's bias as the two tables estimate it, exactly 0 in sweep 1."""
        from .valuefit import fit_stats, mean_table, sweep_targets, trace_stats
        cur = {"a": W_a.clone(), "b": W_b.clone()}             # what the sweep's targets bootstrap from and its residuals are taken against
        new = {"a": W_a, "b": W_b}
        W_mean_old = mean_table(W_a, W_b)
        lt = {"a": sweep_targets(ectx, fl, cur["a"], gamma, lam, r_succ, traced=True, cut=cut, W_val=cur["b"]),
              "b": sweep_targets(ectx, fl, cur["b"], gamma, lam, r_succ, traced=True, cut=cut, W_val=cur["a"])}
        y_mean = (lt["a"]["y"] + lt["b"]["y"]) / 2.0
        report = {}
        for k in vfs:
            report[k] = {"folds": {}}
            for fold, name in enumerate(("a", "b")):
                rows = self._sample_rows(fl, k, fl["env"] % 4 == 2 * fold, by_action=True)
                rep, operands = unit(k, rows, rows.numel(), lt[name]["y"], cur[name], new[name])
                rep = {"n": rep["n"], "delta_norm": rep["delta_norm"], "fit": rep["fit"], "mc": rep["mc"]["fit"]}
                if keep:
                    operands.pop("n_fit")                      # (a fold has no held-out part)
                    rep["operands"] = operands
                report[k]["folds"][name] = rep
        W_mean = mean_table(W_a, W_b)
        for k, rep in report.items():                          # the mean table, judged once both tables of the sweep stand
            rep["n"] = [x + y for x, y in zip(rep["folds"]["a"]["n"], rep["folds"]["b"]["n"])]
            dk = W_mean[k].double() - W_mean_old[k].double()
            rep["delta_norm"] = float(torch.sqrt(torch.sum(dk * dk)))
            halves = [self._sample_rows(fl, k, fl["env"] % 2 == r) for r in (0, 1)]
            q = lambda W: np.concatenate([q_of(ectx, [fl[f][at - 1].contiguous() for f in ("x", "y", "vx", "vy")], W, k,
                                               fl["action"][at].contiguous()) for at in halves])
            at = torch.cat(halves)
            stats = fit_stats(q(W_mean_old), q(W_mean), y_mean[at].cpu().numpy(), y_mc[at.cpu().numpy()], halves[0].numel())
            rep["mc"] = stats.pop("mc")
            rep.update(stats)
            boot, vs, v = (fl["tab0"] == 0, "vs0", "v0") if k == 0 else (fl["tabk"] == k, "vsk", "vk")
            gap = np.concatenate([(t[vs][boot].double() - t[v][boot].double()).cpu().numpy() for t in lt.values()])
            rep["optimism"] = float(np.mean(gap)) if len(gap) else float("nan")
            rep["optimism_n"] = int(boot.sum())
            sets = [trace_stats(t, self._sample_rows(fl, k, fl["env"] >= 0)) for t in lt.values()]
            for name in ("cut_share", "off_greedy", "horizon"):
                rep[name] = float(np.mean([s[name] for s in sets]))
        return report, W_mean, lt

    def fit_values_lstdq(self, n_episodes: int = 4096, epsilon: float = 0.1, seed: Optional[int] = None, vfs=None,
                         ridge: float = 1e-3, rounds: int = 1, apply: bool = False, keep: bool = False, interrupt: bool = False,
                         choose: Optional[str] = None, trajectory=None, weights: Optional[torch.Tensor] = None):
        """Least-squares policy evaluation of the GREEDY policy of the current weights, off-policy from recorded episodes (SPEC §17,
        LSTD-Q): record_episodes() with the current policy, then per value function k of `vfs` (default: all) the items of
        valuefit.td_samples, their greedy next actions a' and TD residuals delta under W^o = W, on the EVEN envs (the odd envs are
        held out) A, b by ScgContext.feature_gram with the action as segment and yv = delta, C by ScgContext.feature_cross_gram on
        the CONT samples with (a, a') as segment, Delta by valuefit.lstdq_solve (a float64 LU of 6480^2, on the device), W_k[a] <-
        float32(W^o_k[a] + Delta_a). Every value function of a round is solved from the same W^o (an option's BOOT samples use the
        root's W^o row). `rounds` = R repeats this on the same samples with W^o <- W^new: least-squares policy iteration.
        Returns (report, W_new): report["rounds"][r]["vf"][k] holds n (fit samples per action), kinds (CONT / BOOT / END counts),
        delta_norm, solve_residual, a_changed (share of samples whose a' differs from the round before; None in round 0) and, for
        "fit" and "held_out", "td" and "mc", each old / new: n, rmse, mean_error of the frozen-policy TD residual and of Q against
        §16.2's Monte-Carlo targets; report["rounds"][r]["W"] is the weights after round r and report["solve_seconds"] lists the
        solves' wall times. `keep` adds per round and k "operands" (rows, kind, r, action, a2, delta, offsets, n_fit, c_index,
        c_offsets, states, next_states, A, b, C, Delta), and report["targets"], report["trajectory"].
        `trajectory`: a kept record to evaluate on instead of recording; `weights`: W^o of the first round instead of W.
        apply=False leaves the agent as evaluate() does; apply=True copies the fitted rows of `vfs` into W and is refused with
        shared weights. Non-finite rows of W^o are refused; a solve that fails raises ScgError and leaves the agent untouched."""
        import time
        from .valuefit import (TD_BOOT, TD_CONT, TD_END, error_stats, greedy_max, lstdq_residual, lstdq_solve, returns_to_go,
                               td_residual, td_samples)
        if apply and self.group is not None:
            raise ScgError("fit_values_lstdq(apply=True) with shared weights: each rank would fit its own copy of W and the "
                           "ranks would part; fit with apply=False and load one rank's result on all of them")
        vfs = list(range(self.n_vf)) if vfs is None else [int(k) for k in vfs]
        if any(not (0 <= k < self.n_vf) for k in vfs):
            raise ValueError(f"vfs must name value functions 0..{self.n_vf - 1}")
        if int(rounds) < 1:
            raise ValueError("rounds must be >= 1")
        W_cur = (self.W if weights is None else weights.to(self.W.device).view_as(self.W)).clone()
        if not bool(torch.isfinite(W_cur[sorted(set(vfs) | {0})]).all()):
            raise ScgError("fit_values_lstdq: the weights to evaluate hold non-finite values")
        c = self.ctx.cfg
        gamma, r_succ = float(c.gamma), float(c.r_option_success)
        if trajectory is None:
            traj, summary = self.record_episodes(n_episodes, epsilon=epsilon, seed=seed, interrupt=interrupt, choose=choose)
        else:
            traj, summary = trajectory, None
        ectx = self._eval_context(int(traj.n), epsilon, seed, None)[0]
        flat = traj.to_numpy()
        tg = returns_to_go(flat, gamma, r_succ)
        dev = self.W.device
        report = {"episodes": summary, "ridge": float(ridge), "gamma": gamma, "rounds": [], "solve_seconds": []}

        def q_all(states, Wk):                                 # Q_k(s_n, .) [5][n] of a sample list, float32 as the kernel gives it
            n = states[0].numel()
            out = np.zeros((NUM_ACTIONS, n), np.float32)
            for i in range(0, n, ectx.n_envs):
                sl = slice(i, i + ectx.n_envs)
                out[:, sl] = ectx.q_values([t[sl].contiguous() for t in states], Wk.contiguous().view(-1)).cpu().numpy()
            return out

        items = {}
        for k in vfs:                                          # what does not change from round to round
            it = td_samples(flat, k, r_succ)
            fit = np.nonzero(it["env"] % 2 == 0)[0]
            fit = fit[np.argsort(flat["action"][it["rows"][fit]], kind="stable")]      # the fit samples by action, (env, row) order within one
            order = np.concatenate([fit, np.nonzero(it["env"] % 2 == 1)[0]])          # ... then the held-out half
            rows = it["rows"][order]
            act = flat["action"][rows].astype(np.int64)
            n_a = np.bincount(act[:len(fit)], minlength=NUM_ACTIONS).astype(np.int64)
            up = lambda at: [torch.from_numpy(np.ascontiguousarray(flat[f][at])).to(dev) for f in ("x", "y", "vx", "vy")]
            items[k] = dict(rows=rows, kind=it["kind"][order], r=it["r"][order], act=act, n_fit=len(fit), n_a=n_a,
                            offsets=np.concatenate([[0], np.cumsum(n_a)]).astype(np.int64), s=up(rows - 1), s2=up(rows),
                            y=tg["y"][rows], A=None, a2=None)

        for rnd in range(int(rounds)):
            W_next = W_cur.clone()
            out = {"vf": {}}
            for k in vfs:
                it = items[k]
                kind, act, n_fit, idx = it["kind"], it["act"], it["n_fit"], np.arange(len(it["rows"]))
                q_sa = q_all(it["s"], W_cur[k])[act, idx]
                qn = q_all(it["s2"], W_cur[k])
                m_k, a2 = greedy_max(qn)
                m_0 = greedy_max(q_all(it["s2"], W_cur[0]))[0] if np.any(kind == TD_BOOT) else np.zeros_like(m_k)
                delta = td_residual(it["r"], kind, gamma, q_sa, m_k, m_0)
                A, b = ectx.feature_gram(it["s"], it["offsets"], torch.from_numpy(delta).to(dev))
                if it["A"] is None:                            # sum phi phi^T does not change: the first round's is kept
                    it["A"] = A
                cont = np.nonzero(kind[:n_fit] == TD_CONT)[0]
                key = NUM_ACTIONS * act[cont] + a2[cont]
                c_index = cont[np.argsort(key, kind="stable")]  # the CONT fit samples by (a, a'), (env, row) order within a pair
                c_off = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=NUM_ACTIONS ** 2))]).astype(np.int64)
                at = torch.from_numpy(c_index).to(dev)
                Cm = ectx.feature_cross_gram([t[at].contiguous() for t in it["s"]], [t[at].contiguous() for t in it["s2"]], c_off)
                Ah, bh = it["A"].cpu().numpy(), b.cpu().numpy()
                Ch = Cm.cpu().numpy().reshape(NUM_ACTIONS, NUM_ACTIONS, NUM_FEATURES, NUM_FEATURES)
                t0 = time.perf_counter()
                Delta = lstdq_solve(Ah, Ch, bh, it["n_a"], gamma, ridge, self.ctx.scale, device=dev)
                report["solve_seconds"].append(time.perf_counter() - t0)
                w_old = W_cur[k].cpu().numpy()
                w_new = (w_old.astype(np.float64) + Delta).astype(np.float32)
                w_new[it["n_a"] == 0] = w_old[it["n_a"] == 0]
                W_next[k] = torch.from_numpy(w_new).to(dev)
                # the same frozen policy under the new weights: a' and the root's m_0 stay W^o's
                q_sa_new = q_all(it["s"], W_next[k])[act, idx]
                delta_new = td_residual(it["r"], kind, gamma, q_sa_new, q_all(it["s2"], W_next[k])[a2, idx], m_0)
                rep = {"n": [int(v) for v in it["n_a"]], "delta_norm": float(np.sqrt(np.sum(Delta * Delta))),
                       "kinds": {name: int(np.sum(kind == v)) for name, v in (("CONT", TD_CONT), ("BOOT", TD_BOOT), ("END", TD_END))},
                       "solve_residual": lstdq_residual(Ah, Ch, bh, it["n_a"], gamma, ridge, self.ctx.scale, Delta),
                       "a_changed": None if it["a2"] is None else (float(np.mean(a2 != it["a2"])) if len(a2) else 0.0)}
                zero = np.zeros(len(idx))
                for name, sl in (("fit", slice(0, n_fit)), ("held_out", slice(n_fit, None))):
                    rep[name] = {"td": {"old": error_stats(delta[sl], zero[sl]), "new": error_stats(delta_new[sl], zero[sl])},
                                 "mc": {"old": error_stats(q_sa[sl], it["y"][sl]), "new": error_stats(q_sa_new[sl], it["y"][sl])}}
                if keep:
                    rep["operands"] = {"rows": it["rows"], "kind": kind, "r": it["r"], "action": act, "a2": a2, "delta": delta,
                                       "offsets": it["offsets"], "n_fit": n_fit, "c_index": c_index, "c_offsets": c_off,
                                       "states": it["s"], "next_states": it["s2"], "A": it["A"], "b": b, "C": Cm, "Delta": Delta}
                it["a2"] = a2
                out["vf"][k] = rep
            W_cur = W_next
            out["W"] = W_cur.clone()
            report["rounds"].append(out)
        if keep:
            report["targets"], report["trajectory"] = tg, traj
        if apply:
            for k in vfs:
                self.W[k].copy_(W_cur[k])
        return report, W_cur

    # ------------------------------------------------------------------ branch rollouts (SPEC §19)
    def branch_returns(self, sources: dict, actions, replicates: int = 8, epsilon: float = 0.1, seed: Optional[int] = None,
                       interrupt: bool = False, choose: Optional[str] = None, steps_per_launch: int = 64) -> BranchResult:
        """Monte-Carlo returns of forced first actions from recorded states (SPEC §19). `sources`: Trajectory.resume_state's dict
        for M states (x, y, vx, vy, option_id, opt_steps, ep_steps, vf_next); `actions` [M][A] uint8, A = 1 .. 5: the first actions
        to force per state; `replicates` = R runs of each. Env (i * A + a) * R + r of a cached context of M A R envs, its global
        env ids from _lib.BRANCH_ID_BASE on (no random stream of a record, whose ids start at 0, is reused), starts in source i's
        whole env state with qcache = Q_vf_next(s, .), takes actions[i][a] on its first step (scg_rollout_branch) and goes on under
        the current policy (W, clf, enabled options, `epsilon`, `interrupt`, `choose`) to the end of the episode: one-episode
        launches without a begin at t0 = 0, spl, 2 spl, ... Returns a BranchResult (g, ret, goal, steps: [M][A][R], from the
        branch step on; g carries no completion bonus). The training run is left alone exactly as evaluate() leaves it."""
        if choose not in (None, "value"):
            raise ValueError(f"choose must be None or 'value', not {choose!r}")
        acts = np.ascontiguousarray(np.asarray(actions, np.uint8))
        if acts.ndim != 2 or not (1 <= acts.shape[1] <= NUM_ACTIONS) or acts.shape[0] < 1 or int(acts.max()) >= NUM_ACTIONS:
            raise ValueError(f"actions must be [M][A] with 1 <= A <= {NUM_ACTIONS} and entries below {NUM_ACTIONS}")
        M, A = (int(v) for v in acts.shape)
        R, spl = int(replicates), int(steps_per_launch)
        if R < 1:
            raise ValueError("replicates must be >= 1")
        if not (1 <= spl <= _lib.ROLLOUT_MAX_STEPS):
            raise ValueError(f"steps_per_launch must be in [1, {_lib.ROLLOUT_MAX_STEPS}]")
        need = ("x", "y", "vx", "vy", "option_id", "opt_steps", "ep_steps", "vf_next")
        src = {f: np.asarray(sources[f]).reshape(-1) for f in need}
        if any(len(v) != M for v in src.values()):
            raise ValueError(f"sources must hold {M} states, one per row of actions")
        vf_next = src["vf_next"].astype(np.int64)
        if np.any(vf_next < 0) or np.any(vf_next >= self.n_vf):
            raise ValueError(f"sources['vf_next'] must name value functions 0..{self.n_vf - 1}")
        n, per = M * A * R, A * R
        seed = int(self.ctx.cfg.seed) if seed is None else int(seed)
        cache = self._branch_ctx                               # one branch context per env count, as the evaluation contexts
        if n not in cache or cache[n][0].cfg.seed != seed:
            if n in cache:
                cache.pop(n)[0].close()
            bctx = ScgContext(n, self.n_options, self.map, device=self.ctx.device.index, seed=seed,
                              env_id_base=_lib.BRANCH_ID_BASE, block_envs=self.ctx.block_envs)
            cache[n] = (bctx, EnvState(n, bctx.device, self.map), EpisodeStats(self.n_vf, n, bctx.device))
        bctx, st, stats = cache[n]
        self._mirror_training(bctx, epsilon)
        stats.zero_()
        dev = bctx.device
        up = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v)).to(dev).to(dt).contiguous()
        s_src = [up(src[f], torch.float32) for f in ("x", "y", "vx", "vy")]
        q_src = torch.zeros((NUM_ACTIONS, M), dtype=torch.float32, device=dev)
        for k in sorted(set(vf_next.tolist())):                # qcache = Q_vf_next(s, .), as the step before left it
            at = torch.from_numpy(np.nonzero(vf_next == k)[0]).to(dev)
            q_src[:, at] = bctx.q_values([t[at].contiguous() for t in s_src], self.W[k].contiguous().view(-1))
        for dst, v in zip((st.x, st.y, st.vx, st.vy), s_src):
            dst.copy_(v.repeat_interleave(per))
        for f in ("option_id", "opt_steps", "ep_steps"):
            getattr(st, f).copy_(up(src[f], torch.int32).repeat_interleave(per))
        st.qcache.copy_(q_src.repeat_interleave(per, dim=1))
        st.action.zero_(); st.reward.zero_(); st.done.zero_()
        audit = GateAudit(n, dev)                              # disc_ret = 0, disc_g = 1, disc_final = NaN until the episode ends
        first = up(acts.reshape(-1), torch.uint8).repeat_interleave(R).contiguous()
        for i in range(-(-int(self.ctx.cfg.max_episode_steps) // spl)):
            bctx.rollout(st, self.W, self.clf, self.enabled_mask, i * spl, spl, stats, one_episode=True, interrupt=interrupt,
                         choose=choose, audit=audit, first_action=first if i == 0 else None)
        shape = (M, A, R)
        ep0 = np.repeat(src["ep_steps"].astype(np.int64), per).reshape(shape)
        res = BranchResult(acts, audit.disc_final.cpu().numpy().reshape(shape), stats.ret_sum.cpu().numpy().reshape(shape),
                           stats.goals.cpu().numpy().reshape(shape) > 0,
                           stats.len_sum.cpu().numpy().astype(np.int64).reshape(shape) - ep0)
        res.qcache = q_src.cpu().numpy().T.copy()              # [M][5]: what the source's policy saw
        res.finished = stats.finished.cpu().numpy().reshape(shape) != 0
        return res

    def branch_audit(self, trajectory=None, n_states: int = 1024, replicates: int = 8, actions: str = "all", vfs=None,
                     epsilon: float = 0.1, seed: Optional[int] = None, n_episodes: int = 4096, interrupt: bool = False,
                     choose: Optional[str] = None, steps_per_launch: int = 64) -> dict:
        """How much of a value function's error is noise, and is its greedy action the best one (SPEC §19)? Records episodes as
        fit_values_to_returns does (or takes its `trajectory`), then per value function k of `vfs` (default: all) draws `n_states`
        rows (fewer where there are fewer) uniformly, with a generator seeded by `seed`, from the held-out (odd) envs' rows with
        vf = k — the state distribution §16's held-out RMSE is over — rebuilds each row's env state (Trajectory.resume_state) and
        runs branch_returns from it: `actions` = "taken": the recorded action only; "all": all five. `replicates` must be even, >= 2.
        Returns {"trajectory", "vf": {k: {"n", "rows", "taken", "g_recorded", "spread", "actions" (with "all"), "result"}}}:
        "spread" is BranchResult.spread of the recorded action against the record's own return-to-go (§16.2's g, "g_recorded"),
        "actions" BranchResult.action_table of a_W = the first maximum of the source's qcache, "result" the BranchResult, "rows"
        the sampled rows' (env, row), "taken" their recorded actions; "trajectory" is the record. A branch's g carries no
        completion bonus, so with r_option_success != 0 a report for k >= 1 is refused. All arithmetic is host float64, in state
        order. The training run is left alone exactly as evaluate() leaves it."""
        from .valuefit import returns_to_go
        if actions not in ("all", "taken"):
            raise ValueError(f"actions must be 'all' or 'taken', not {actions!r}")
        R = int(replicates)
        if R < 2 or R % 2:
            raise ValueError(f"replicates must be even and >= 2, not {replicates}")
        if int(n_states) < 1:
            raise ValueError("n_states must be >= 1")
        vfs = list(range(self.n_vf)) if vfs is None else [int(k) for k in vfs]
        if any(not (0 <= k < self.n_vf) for k in vfs):
            raise ValueError(f"vfs must name value functions 0..{self.n_vf - 1}")
        c = self.ctx.cfg
        if float(c.r_option_success) != 0.0 and any(k >= 1 for k in vfs):
            raise ScgError("branch_audit: r_option_success != 0: a branch's return carries no completion bonus, so it is not "
                           "SPEC §16.2's target of an option's value function; report vfs=[0] only")
        if trajectory is None:
            traj, _ = self.record_episodes(n_episodes, epsilon=epsilon, seed=seed, interrupt=interrupt, choose=choose)
        else:
            traj = trajectory
        flat = traj.to_numpy()
        tg = returns_to_go(flat, float(c.gamma), float(c.r_option_success))
        off = flat["offsets"]
        env = np.repeat(np.arange(traj.n), np.diff(off))
        row = np.arange(int(off[-1])) - off[:-1][env]
        rng = np.random.default_rng(int(c.seed) if seed is None else int(seed))
        report = {"replicates": R, "actions": actions, "trajectory": traj, "vf": {}}
        for k in vfs:
            rows = np.nonzero(tg["sample"] & (flat["vf"] == k) & (env % 2 == 1))[0]
            if len(rows) > int(n_states):
                rows = np.sort(rng.choice(rows, int(n_states), replace=False))
            taken = flat["action"][rows].astype(np.uint8)
            rep = {"n": int(len(rows)), "rows": (env[rows], row[rows]), "taken": taken.astype(np.int64), "g_recorded": tg["g"][rows]}
            if len(rows):
                acts = np.tile(np.arange(NUM_ACTIONS, dtype=np.uint8), (len(rows), 1)) if actions == "all" else taken[:, None]
                res = self.branch_returns(traj.resume_state(env[rows], row[rows]), acts, R, epsilon, seed, interrupt, choose,
                                          steps_per_launch)
                rep["spread"] = res.spread(tg["g"][rows], column=taken.astype(np.int64) if actions == "all" else 0)
                if actions == "all":
                    rep["actions"] = res.action_table(np.argmax(res.qcache, axis=1))
                rep["result"] = res
            report["vf"][k] = rep
        return report

    def fit_values_to_branches(self, trajectory=None, n_states: int = 8192, n_held: int = 2048, replicates: int = 8, vfs=None,
                               ridge: float = 1e-3, epsilon: float = 0.1, seed: Optional[int] = None, n_episodes: int = 4096,
                               apply: bool = False, keep: bool = False, interrupt: bool = False, choose: Optional[str] = None,
                               steps_per_launch: int = 64, weighting=None, tau2: Optional[float] = None, branches: Optional[dict] = None):
        """Fit every action's Q_k to fresh Monte-Carlo branch returns of ALL five actions from the same states (SPEC §20): one Gram,
        a right-hand side per action. Records episodes as branch_audit does (or takes its `trajectory`), then per value function k
        of `vfs` (default: all), with a generator seeded by `seed`, draws `n_states` rows of the EVEN envs' step rows with vf = k
        (the fit half) and then `n_held` of the ODD envs' (the held-out half), fewer where there are fewer, each in (env, row)
        order; rebuilds the rows' env states (Trajectory.resume_state) and runs branch_returns from them with all five first
        actions, `replicates` each. With gbar the replicate means and Q^old the result's qcache (valuefit.branch_targets): on the
        fit half (A, B) = ScgContext.feature_gram_targets(states, [0, n_fit], D), D[a] = float32(gbar[:, a] - Q^old[:, a]); Delta =
        valuefit.ridge_solve_shared; W_new[k][a] = float32(W_k^old[a] + Delta[a]). A value function without fit states keeps its
        rows bit for bit. This fits Q of the epsilon-greedy policy that ran the branches; acting greedily on W_new is a step of
        policy improvement.
        Returns (report, W_new): W_new a copy of W with the fitted rows; report["vf"][k] holds n_fit, n_held, delta_norm and, for
        "fit" and "held_out": old / new (valuefit.error_stats of Q(s_i, a) against gbar[i][a] over all (i, a)), per_action (the
        same per action), target_se = sqrt(mean se2) (the RMSE a perfect Q^pi would still show against these means) and greedy
        (valuefit.greedy_table: agreement_old / _new, changed, one_step_gain and its standard error; unbiased on the held-out
        half, whose replicates W_new never saw). `keep` adds report["vf"][k]["operands"] (states, D, A, B, delta, rows, n_fit,
        gbar, se2, q_old, q_new, result) and report["trajectory"].
        `weighting` (SPEC §22): None is the fit above, untouched. "precision" weights every fit state by the precision of its
        targets, w = valuefit.precision_weights(se2 of the fit half, tau2), and forms (A, B) = ScgContext.feature_gram_weighted(states,
        [0, n_fit], valuefit.root_weights(w), D): one Gram, five targets, ridge_solve_shared as above. "precision_per_action" gives
        every action its own weights (per_action=True): the fit states five times over as five segments with one target, the
        segment of action a under column a of the weights, and valuefit.ridge_solve per action. An array [n_fit] or [n_fit][5] is
        taken as w itself (valuefit.normalise_weights: mean 1 per column). With w = 1 everywhere (replicates = 1: se2 = 0) W_new has
        the unweighted fit's bits. The report gains "weighting" ("given" for an array) and "tau2" (the argument) and, per weighted
        value function, "tau2" (the value used) and "effective_n" = (sum w)^2 / sum w^2 (a list of five per action); old / new / per_action / greedy stay
        UNWEIGHTED statistics against gbar on both halves: one yardstick for every weighting. `keep` adds w and rw to the operands.
        `branches`: an earlier keep=True report; its trajectory, rows, states and BranchResults are reused and no rollout runs, so
        that only the regression differs between two calls: several weightings on the SAME returns.
        Refused: r_option_success != 0 with any k >= 1 (as branch_audit), apply=True with shared weights (as
        fit_values_to_returns), replicates < 1, n_states < 1, n_held < 0; ValueError for an unknown `weighting` string, weights of
        a wrong shape, negative or non-finite, and a `branches` report without a trajectory or without the operands of a value
        function of `vfs`. apply=False leaves the agent as evaluate() does; apply=True copies the fitted rows of `vfs` into W."""
        from .valuefit import returns_to_go
        if isinstance(weighting, str) and weighting not in ("precision", "precision_per_action"):
            raise ValueError(f"weighting must be None, 'precision', 'precision_per_action' or an array of weights, not {weighting!r}")
        if int(replicates) < 1:
            raise ValueError("replicates must be >= 1")
        if int(n_states) < 1:
            raise ValueError("n_states must be >= 1")
        if int(n_held) < 0:
            raise ValueError("n_held must be >= 0")
        if apply and self.group is not None:
            raise ScgError("fit_values_to_branches(apply=True) with shared weights: each rank would fit its own copy of W and the "
                           "ranks would part; fit with apply=False and load one rank's result on all of them")
        vfs = list(range(self.n_vf)) if vfs is None else [int(k) for k in vfs]
        if any(not (0 <= k < self.n_vf) for k in vfs):
            raise ValueError(f"vfs must name value functions 0..{self.n_vf - 1}")
        c = self.ctx.cfg
        if float(c.r_option_success) != 0.0 and any(k >= 1 for k in vfs):
            raise ScgError("fit_values_to_branches: r_option_success != 0: a branch's return carries no completion bonus, so it is "
                           "not SPEC §16.2's target of an option's value function; fit vfs=[0] only")
        if branches is not None:                               # an earlier report's record and returns: only the regression runs
            if not isinstance(branches, dict) or "trajectory" not in branches or any(
                    k not in branches.get("vf", {}) or (branches["vf"][k]["n_fit"] and "operands" not in branches["vf"][k]) for k in vfs):
                raise ValueError("branches must be a fit_values_to_branches(keep=True) report that holds every value function of vfs")
            return self._fit_branches(branches["trajectory"], None, None, vfs, branches, n_states, n_held, replicates, ridge, epsilon, seed,
                                      apply, keep, interrupt, choose, steps_per_launch, weighting, tau2)
        if trajectory is None:
            traj, _ = self.record_episodes(n_episodes, epsilon=epsilon, seed=seed, interrupt=interrupt, choose=choose)
        else:
            traj = trajectory
        flat = traj.to_numpy()
        tg = returns_to_go(flat, float(c.gamma), float(c.r_option_success))
        return self._fit_branches(traj, flat, tg, vfs, None, n_states, n_held, replicates, ridge, epsilon, seed, apply, keep, interrupt,
                                  choose, steps_per_launch, weighting, tau2)

    def _fit_branches(self, traj, flat, tg, vfs, branches, n_states, n_held, replicates, ridge, epsilon, seed, apply, keep, interrupt,
                      choose, steps_per_launch, weighting, tau2):
        """fit_values_to_branches behind its checks: per value function the rows, the branch returns (or `branches`' kept ones), the
        Gram under `weighting`, the solve and the report."""
        from .valuefit import (branch_targets, error_stats, greedy_table, normalise_weights, precision_weights, ridge_solve,
                               ridge_solve_shared, root_weights)
        c = self.ctx.cfg
        if branches is None:
            off = flat["offsets"]
            env = np.repeat(np.arange(traj.n), np.diff(off))
            row = np.arange(int(off[-1])) - off[:-1][env]
            rng = np.random.default_rng(int(c.seed) if seed is None else int(seed))
        dev = self.W.device
        W_new = self.W.clone()
        report = {"replicates": int(replicates), "ridge": float(ridge), "vf": {},
                  "weighting": weighting if weighting is None or isinstance(weighting, str) else "given",
                  "tau2": None if tau2 is None else float(tau2)}
        if keep:
            report["trajectory"] = traj
        for k in vfs:
            if branches is not None:
                n_fit, n_hld = int(branches["vf"][k]["n_fit"]), int(branches["vf"][k]["n_held"])
            else:
                halves = []
                for parity, want in ((0, int(n_states)), (1, int(n_held))):
                    rows = np.nonzero(tg["sample"] & (flat["vf"] == k) & (env % 2 == parity))[0]
                    if len(rows) > want:
                        rows = np.sort(rng.choice(rows, want, replace=False)) if want else rows[:0]
                    halves.append(rows)
                n_fit, n_hld = len(halves[0]), len(halves[1])
                rows = np.concatenate(halves)
            rep = {"n_fit": int(n_fit), "n_held": int(n_hld), "delta_norm": 0.0}
            report["vf"][k] = rep
            if n_fit == 0:                                     # nothing to fit: the rows of W_k stay, and there is no Q^new to judge
                continue
            if branches is not None:
                op = branches["vf"][k]["operands"]
                res, states, kept_rows = op["result"], op["states"], op["rows"]
                # the side context the branches ran on where the agent still holds it; the Gram and q_values need no particular one
                ectx = self._branch_ctx[res.g.size][0] if res.g.size in self._branch_ctx else self.ctx
            else:
                # the fit half's states first: its branch envs, and so its returns, do not depend on n_held
                res = self.branch_returns(traj.resume_state(env[rows], row[rows]), np.tile(np.arange(NUM_ACTIONS, dtype=np.uint8), (len(rows), 1)),
                                          int(replicates), epsilon, seed, interrupt, choose, steps_per_launch)
                ectx = self._branch_ctx[res.g.size][0]           # the side context the branches ran on: 5 R envs per state
                states = [torch.from_numpy(np.ascontiguousarray(flat[f][rows - 1])).to(dev) for f in ("x", "y", "vx", "vy")]
                kept_rows = (env[rows], row[rows])
            gbar, se2, D = branch_targets(res.g, res.qcache)
            fit_states = [t[:n_fit].contiguous() for t in states]
            D_fit = torch.from_numpy(np.ascontiguousarray(D[:, :n_fit])).to(dev)
            w = rw = None
            if weighting is None:
                A, B = ectx.feature_gram_targets(fit_states, [0, n_fit], D_fit)
                delta = ridge_solve_shared(A[0].cpu().numpy(), B[0].cpu().numpy(), n_fit, ridge, self.ctx.scale)
            else:
                if isinstance(weighting, str):
                    w, rep["tau2"] = precision_weights(se2[:n_fit], tau2, per_action=weighting == "precision_per_action")
                else:
                    w = np.asarray(weighting, np.float64)
                    if w.shape not in ((n_fit,), (n_fit, NUM_ACTIONS)):
                        raise ValueError(f"weighting must be [{n_fit}] or [{n_fit}][{NUM_ACTIONS}] for value function {k}, not {w.shape}")
                    w = normalise_weights(w)
                rw = torch.from_numpy(root_weights(w)).to(dev)
                sw, sw2 = np.cumsum(w, axis=0)[-1], np.cumsum(w * w, axis=0)[-1]
                rep["effective_n"] = (sw * sw / sw2).tolist() if w.ndim == 2 else float(sw * sw / sw2)
                if w.ndim == 1:                                # one Gram under the states' weights, a target per action
                    A, B = ectx.feature_gram_weighted(fit_states, [0, n_fit], rw, D_fit)
                    delta = ridge_solve_shared(A[0].cpu().numpy(), B[0].cpu().numpy(), n_fit, ridge, self.ctx.scale)
                else:                                          # segment a: the fit states under action a's weights, D[a] its one target
                    A, B = ectx.feature_gram_weighted([t.repeat(NUM_ACTIONS) for t in fit_states], n_fit * np.arange(NUM_ACTIONS + 1),
                                                      rw.T.contiguous().view(-1), D_fit.view(1, -1))
                    delta = ridge_solve(A.cpu().numpy(), B[:, 0].cpu().numpy(), [n_fit] * NUM_ACTIONS, ridge, self.ctx.scale)
            w_old = self.W[k].cpu().numpy()
            W_new[k] = torch.from_numpy((w_old.astype(np.float64) + delta).astype(np.float32)).to(dev)
            q_old = res.qcache
            q_new = np.zeros_like(q_old)
            for i in range(0, n_fit + n_hld, ectx.n_envs):     # (a branch context holds 5 R envs per state: one pass)
                sl = slice(i, i + ectx.n_envs)
                q_new[sl] = ectx.q_values([t[sl].contiguous() for t in states], W_new[k].contiguous().view(-1)).cpu().numpy().T
            rep["delta_norm"] = float(np.sqrt(np.sum(delta * delta)))
            for name, sl in (("fit", slice(0, n_fit)), ("held_out", slice(n_fit, None))):
                rep[name] = {"old": error_stats(q_old[sl].reshape(-1), gbar[sl].reshape(-1)),
                             "new": error_stats(q_new[sl].reshape(-1), gbar[sl].reshape(-1)),
                             "per_action": [{"old": error_stats(q_old[sl, a], gbar[sl, a]), "new": error_stats(q_new[sl, a], gbar[sl, a])}
                                            for a in range(NUM_ACTIONS)],
                             "target_se": float(np.sqrt(np.mean(se2[sl]))) if se2[sl].size else float("nan"),
                             "greedy": greedy_table(gbar[sl], q_old[sl], q_new[sl])}
            if keep:
                rep["operands"] = {"states": states, "D": D, "A": A, "B": B, "delta": delta, "rows": kept_rows, "n_fit": n_fit,
                                   "gbar": gbar, "se2": se2, "q_old": q_old, "q_new": q_new, "result": res}
                if w is not None:
                    rep["operands"].update(w=w, rw=rw)
        if apply:
            for k in vfs:
                self.W[k].copy_(W_new[k])
        return report, W_new

    def _mirror_training(self, side: ScgContext, epsilon: float) -> None:
        """Copy the training run's settings into a side context (evaluation, trials): its hyper-parameters (epsilon aside),
        parents and gestation mask — classifiers in use, no success counts kept; its own state, t and counters untouched."""
        side.set_hparams(**dict({k: getattr(self.ctx.cfg, k) for k in ScgContext._HPARAMS}, epsilon=float(epsilon)))
        side.set_option_parents([int(v) for v in self.ctx.parents])
        side.set_gestation(self.gest_mask, counters=False)

    # ------------------------------------------------------------------ option trials (SPEC §9)
    def option_trials(self, option, x, y, vx=None, vy=None, epsilon: float = 0.0, seed: Optional[int] = None,
                      record: Optional[int] = None, clf=None):
        """Run option `option` (an int, or one id per start state) from each start state (x, y, vx, vy; velocities default to
        zero) until it terminates, with the current W, clf and enabled / gestating options, weights frozen (SPEC §9). Returns a
        TrialResult (outcome, steps, ret, disc_ret, v0, end state; summary() per option). Runs on a separate cached context
        at t0 = 0: W, state, t, the training context's env order, trace ring and counters are untouched. With `record` (rows
        per entry) every step is recorded (SPEC §10) into res.trajectory, a Trajectory over all entries. `clf`: a classifier table
        [n_vf, 8] to run the trials under instead of the agent's (SPEC §24.3's fixed-point lines); it is read only."""
        dev = self.W.device
        x, y = self._f32(x), self._f32(y)
        n = x.numel()
        vx = torch.zeros(n, dtype=torch.float32, device=dev) if vx is None else self._f32(vx)
        vy = torch.zeros(n, dtype=torch.float32, device=dev) if vy is None else self._f32(vy)
        opt = torch.full((n,), int(option), dtype=torch.int32, device=dev) if isinstance(option, int) \
            else torch.as_tensor(option, dtype=torch.int32).to(dev).contiguous().view(-1)
        seed = int(self.ctx.cfg.seed) if seed is None else int(seed)
        tc = self._trial_ctx                 # the one cached context trials run on, replaced when another seed is asked for
        if tc is None or tc.cfg.seed != seed:
            if tc is not None:
                tc.close()
            tc = self._trial_ctx = ScgContext(1, self.n_options, self.map, device=self.ctx.device.index, seed=seed,
                                              env_id_base=0, block_envs=self.ctx.block_envs)
        self._mirror_training(tc, epsilon)
        res = TrialResult(n, opt, dev)
        traj = None if record is None else Trajectory(n, int(record), 0, dev, n_vf=self.n_vf)
        table = self.clf if clf is None else torch.as_tensor(clf, dtype=torch.float32).to(dev).contiguous()
        if tuple(table.shape) != tuple(self.clf.shape):
            raise ValueError(f"clf must be {list(self.clf.shape)}, not {tuple(table.shape)}")
        tc.option_trials(x, y, vx, vy, res.option, self.W.view(-1), table.view(-1), self.enabled_mask, 0, res, record=traj)
        if traj is not None:
            res.trajectory = traj.append()
        return res

    def _f32(self, v) -> torch.Tensor:
        """`v` as a flat, contiguous float32 tensor on the agent's device."""
        return torch.as_tensor(v, dtype=torch.float32).to(self.W.device).contiguous().view(-1)

    def _start_states(self, states, n_states: int, seed: int):
        """(x, y, vx, vy) as float32 device tensors: from `states` ((x, y) or (x, y, vx, vy)), else n_states map.sample_free
        positions drawn with `seed`; missing velocities are zero."""
        if states is None:
            pos = self.map.sample_free(int(n_states), np.random.default_rng(seed))
            states = (pos[:, 0], pos[:, 1])
        st = [self._f32(v) for v in states]
        if len(st) not in (2, 4) or any(v.numel() != st[0].numel() for v in st):
            raise ValueError("states must be (x, y) or (x, y, vx, vy) of one length")
        if len(st) == 2:
            st += [torch.zeros_like(st[0]), torch.zeros_like(st[0])]
        return st

    def initiation_report(self, k: int, states=None, n_states: int = 8192, seed: int = 0, classifier=None) -> dict:
        """Does initiation set k hold exactly the states from which option k reaches its target? Trials of option k (greedy)
        from `states` ((x, y) or (x, y, vx, vy); default: n_states map.sample_free positions at rest, drawn with `seed`), each
        start classified by in_k(s0) — or, with `classifier` (an initfit.FourierClassifier, SPEC §23.3), by it: a reporting
        instrument, the trials themselves run with in_k as ever. Returns tp / fp / fn / tn (predicted in I_k x trial
        succeeded), precision, recall, log_loss (the mean log-loss of the classifier's logits against the outcomes: in_k's from
        ScgContext.classifier_logits, SPEC §24.2), success_in / success_out (success rate inside / outside the predicted set; NaN when
        empty), outcomes (count per outcome) and, per entry, trials (the TrialResult), predicted (uint8) and states (x, y, vx, vy)."""
        if not (1 <= k <= self.n_options) or not ((self.enabled_mask | self.gest_mask) >> k) & 1:
            raise ValueError(f"option {k} is not enabled or gestating")
        xs, ys, vxs, vys = self._start_states(states, n_states, seed)
        res = self.option_trials(k, xs, ys, vxs, vys)
        if classifier is None:
            pred = self._trial_ctx.classifier_predict(xs, ys, self.clf[k].contiguous())
            z = self._trial_ctx.classifier_logits(xs, ys, self.clf[k].contiguous())
        else:
            pred = classifier.predict(self._trial_ctx, (xs, ys, vxs, vys))
            z = classifier.logits(self._trial_ctx, (xs, ys, vxs, vys))
        oc = res.outcome.cpu().numpy()
        st = initfit.classification_stats(pred.cpu().numpy(), oc == _lib.TRIAL_SUCCESS, z.cpu().numpy())
        tp, fp, fn, tn = st["tp"], st["fp"], st["fn"], st["tn"]
        nan = float("nan")
        return {
            "option": int(k), "n": int(oc.size),
            "tp": tp, "fp": fp, "fn": fn, "tn": tn,
            "precision": st["precision"],
            "recall": st["recall"],
            "log_loss": st["log_loss"],
            "success_in": tp / (tp + fp) if tp + fp else nan,
            "success_out": fn / (fn + tn) if fn + tn else nan,
            "outcomes": {name: int(np.sum(oc == code)) for code, name in OUTCOMES.items()},
            "trials": res, "predicted": pred,
            "states": (xs, ys, vxs, vys),
        }

    def fit_initiation_fourier(self, k: int, states=None, n_states: int = 8192, order: int = 3, features: str = "state",
                               ridge: float = 1e-3, held_out: float = 0.5, seed: int = 0, trials: Optional[dict] = None):
        """SPEC §23.3: fit a Fourier-basis classifier of order `order` on the `features` ("state": all of the basis, "position":
        the features without velocity) to "option k started here reaches its target". Greedy trials of option k from `states`
        as initiation_report draws or takes them (`trials`: an earlier report of this method or of initiation_report for option k,
        whose states and outcomes are taken over, no trial run); the fit (initfit.irls_fit) on the even-indexed states
        (held_out = 0.5; 0: on all of them). Returns (FourierClassifier, report): report["fit"] and report["held_out"] hold, for
        their half, "n", "fourier" and "shipped" — initfit.classification_stats of the new classifier (with its log-loss) and of
        SPEC §4.1's in_k on the same states —; "history" / "reason" are the fit's, "trials" / "states" / "predicted" /
        "shipped_predicted" per entry. A reporting instrument: runs on the trial context, writes nothing to W, clf, the env state
        or the training context's order."""
        if held_out not in (0, 0.0, 0.5):
            raise ValueError("held_out must be 0.5 (fit on the even-indexed states) or 0 (fit on all)")
        if trials is None:
            trials = self.initiation_report(k, states, n_states, seed)
        elif int(trials["option"]) != int(k):
            raise ValueError(f"trials= is a report of option {trials['option']}, not of option {k}")
        st = tuple(trials["states"])
        ok = (trials["trials"].outcome == _lib.TRIAL_SUCCESS)
        tc = self._trial_ctx
        n = st[0].numel()
        fit_rows = torch.arange(0, n, 2 if held_out else 1, device=ok.device)
        held_rows = torch.arange(1, n, 2, device=ok.device) if held_out else fit_rows
        take = lambda rows: [t[rows].contiguous() for t in st]
        w, history, reason = initfit.irls_fit(tc, order, take(fit_rows), ok[fit_rows], mask=features, ridge=ridge)
        clf = initfit.FourierClassifier(order, features, w)
        z = clf.logits(tc, st)
        pred = (z > 0).to(torch.uint8)
        shipped = trials.get("shipped_predicted")
        if shipped is None:
            shipped = tc.classifier_predict(st[0], st[1], self.clf[k].contiguous())
        z_h, pred_h, ship_h, ok_h = z.cpu().numpy(), pred.cpu().numpy(), shipped.cpu().numpy(), ok.cpu().numpy()
        report = {"option": int(k), "n": int(n), "order": int(order), "features": str(features), "ridge": float(ridge),
                  "held_out": float(held_out), "history": history, "reason": reason, "iterations": len(history) - 1,
                  "trials": trials["trials"], "states": st, "predicted": pred, "shipped_predicted": shipped}
        for name, rows in (("fit", fit_rows), ("held_out", held_rows)):
            r = rows.cpu().numpy()
            report[name] = {"n": int(r.size), "fourier": initfit.classification_stats(pred_h[r], ok_h[r], z_h[r]),
                            "shipped": initfit.classification_stats(ship_h[r], ok_h[r])}
        return clf, report

    def refine_initiation(self, k: int, states=None, n_states: int = 8192, iters: int = 400, lr: float = 3.0,
                          l2: float = 1e-4, seed: int = 0):
        """Refine initiation set k from option k's own executions (Konidaris & Barto 2009): trials from `states` (as in
        initiation_report) label each start state positive iff the trial ended in SUCCESS; classifier k is then fitted,
        starting from its current row, on the option's collected examples (if any are held) followed by the trial-labelled
        states (scg_fit_initiation). Returns (report before, report after), the second from new trials with the refitted
        classifier on the same states. Not available on a sharded agent."""
        if self.group is not None:
            raise ValueError("refine_initiation is not available on a sharded agent")
        before = self.initiation_report(k, states, n_states, seed)
        xs, ys, vxs, vys = before["states"]
        lab = (before["trials"].outcome == _lib.TRIAL_SUCCESS).to(torch.uint8)
        xy = torch.stack((xs, ys), 1)
        if k in self._ex:
            ex_xy, ex_lab = self.examples(k)
            xy, lab = torch.cat((ex_xy, xy)), torch.cat((ex_lab, lab))
        self.options[k].initiation_classifier.fit(xy.contiguous(), lab.contiguous(), iters=iters, lr=lr, l2=l2, warm_start=True)
        after = self.initiation_report(k, (xs, ys, vxs, vys))
        return before, after

    def improve_initiation(self, options=None, states=None, n_states: int = 8192, iters: int = 400, lr: float = 3.0,
                           l2: float = 1e-4, eval_epsilons=(0.0,), criterion: str = "discounted", z: float = 2.0, n_eval: int = 4096,
                           seed: Optional[int] = None, interrupt: bool = False, choose: Optional[str] = None, apply: bool = False):
        """A safeguarded refit of the initiation classifiers (SPEC §24.3), improve_policy's counterpart for in_k. (1) ONE
        option_trials launch runs each of `options` (default: every enabled one) from `states` (as initiation_report draws or takes
        them) under the shipped table; a trial that ends in SUCCESS labels its start positive. (2) Each row k is refitted on the
        even-indexed states by initfit.refit_quadratic (iters, lr, l2); an option whose fit half holds one class only is skipped.
        report["options"][i] holds "option", "n", "successes", "skipped" (None or the reason) and, on the odd-indexed states,
        "shipped" and "refitted": initfit.classification_stats with the log-loss of the row's logits. (3) initfit.candidate_tables'
        tables at each of `eval_epsilons` are evaluated in ONE evaluate_policies run of n_eval episodes each under the agent's W
        (common start states and draws; `interrupt`, `choose` as for evaluate()). (4) initfit.choose_table decides at
        eval_epsilons[0]. (5) One more trial launch on the same states under the table of every refitted row reports, in
        report["fixed_point"], each option's success rate and outcomes next to those under the shipped table (a replaced row k
        moves the target of k's children and the states k is tried from); no second refit. Returns (report, clf_chosen):
        report["candidates"] rows of {"label", "epsilon", "summary", "paired"} (paired: against "shipped" at the same epsilon),
        "chosen" (a label; "shipped" when nothing is accepted), "accepted", "criterion", "z"; clf_chosen a copy of the chosen
        table. apply=True copies it into clf when accepted; refused on a sharded agent. ValueError for an option that is not
        enabled, no epsilon, an unknown criterion, or more candidates x epsilons than a population holds. With apply=False the
        agent is left as evaluate() leaves it."""
        if apply and self.group is not None:
            raise ValueError("improve_initiation(apply=True) is not available on a sharded agent")
        if criterion not in ("discounted", "return", "success"):
            raise ValueError(f"criterion must be 'discounted', 'return' or 'success', not {criterion!r}")
        eps = [float(v) for v in eval_epsilons]
        if not eps:
            raise ValueError("improve_initiation needs at least one epsilon")
        enabled = [k for k in range(1, self.n_options + 1) if (self.enabled_mask >> k) & 1]
        opts = enabled if options is None else sorted({int(k) for k in options})
        if not opts or any(k not in enabled for k in opts):
            raise ValueError(f"options must name enabled options (enabled: {enabled}), not {opts}")
        n_max = 1 + len(opts) + (1 if len(opts) >= 2 else 0)
        if n_max * len(eps) > _lib.POP_MAX:
            raise ValueError(f"{n_max} candidate tables x {len(eps)} epsilons are more than the {_lib.POP_MAX} policies of one population")
        xs, ys, vxs, vys = self._start_states(states, n_states, 0 if seed is None else int(seed))
        n, K = xs.numel(), len(opts)
        opt_ids = torch.tensor(opts, dtype=torch.int32, device=xs.device).repeat_interleave(n)

        def trial_outcomes(table):
            """outcome [K][n] (host) of ONE launch: option opts[i] from every state, under `table`."""
            res = self.option_trials(opt_ids, xs.repeat(K), ys.repeat(K), vxs.repeat(K), vys.repeat(K), seed=seed, clf=table)
            return res.outcome.cpu().numpy().reshape(K, n)

        oc = trial_outcomes(None)
        tc = self._trial_ctx
        rows, opt_rows = {}, []
        for i, k in enumerate(opts):
            ok = oc[i] == _lib.TRIAL_SUCCESS
            rep = {"option": int(k), "n": int(n), "successes": int(ok.sum()), "skipped": None,
                   "outcomes": {name: int(np.sum(oc[i] == code)) for code, name in OUTCOMES.items()}}
            opt_rows.append(rep)
            if ok[0::2].size == 0 or ok[0::2].all() or not ok[0::2].any():
                rep["skipped"] = "the fit half holds one class only"
                continue
            w = initfit.refit_quadratic(tc, self.clf[k], torch.stack((xs[0::2], ys[0::2]), 1), torch.from_numpy(ok[0::2].copy()),
                                        iters, lr, l2)
            rows[k] = w
            xh, yh = xs[1::2].contiguous(), ys[1::2].contiguous()
            for name, w8 in (("shipped", self.clf[k].contiguous()), ("refitted", w)):
                rep[name] = initfit.classification_stats(tc.classifier_predict(xh, yh, w8).cpu().numpy(), ok[1::2],
                                                         tc.classifier_logits(xh, yh, w8).cpu().numpy())
        tables = initfit.candidate_tables(self.clf, rows)
        n_tab, per_eps = len(tables), len(eps)
        stack = torch.stack([t for _, t in tables])
        summaries, _, envs = self.evaluate_policies(self.W, np.repeat(np.asarray(eps, np.float32), n_tab), None, n_episodes=int(n_eval),
                                                    seed=seed, interrupt=bool(interrupt), choose=choose, per_env=True,
                                                    clf=stack.repeat(per_eps, 1, 1))
        cands = [{"label": tables[i][0], "epsilon": eps[e], "summary": summaries[e * n_tab + i],
                  "paired": paired_differences(envs[e * n_tab + i], envs[e * n_tab])} for e in range(per_eps) for i in range(n_tab)]
        pick = initfit.choose_table(cands[:n_tab], criterion, z)
        clf_chosen = dict(tables)[pick["chosen"]].clone()
        fixed = None
        if rows:                                               # the table of every refitted row: "all", or the one fitted k
            oc2 = trial_outcomes(tables[-1][1])
            fixed = [{"option": int(k), "table": tables[-1][0],
                      "shipped": {"success_rate": float(np.mean(oc[i] == _lib.TRIAL_SUCCESS)), "outcomes": opt_rows[i]["outcomes"]},
                      "refitted": {"success_rate": float(np.mean(oc2[i] == _lib.TRIAL_SUCCESS)),
                                   "outcomes": {name: int(np.sum(oc2[i] == code)) for code, name in OUTCOMES.items()}}}
                     for i, k in enumerate(opts)]
        if apply and pick["accepted"]:
            self.clf.copy_(clf_chosen)
        return {"options": opt_rows, "candidates": cands, "chosen": pick["chosen"], "accepted": pick["accepted"],
                "criterion": criterion, "z": float(z), "fixed_point": fixed}, clf_chosen

    def fit_gate(self, n_record: int = 256, n_states: int = 4096, replicates: int = 4, epsilon: float = 0.1, ridge: float = 1e-3,
                 min_offers: int = 256, seed: Optional[int] = None):
        """What is entering worth, as a function of the state (SPEC §25.3)? record_episodes(n_record, epsilon, seed) gives the
        states at which offers happen (Trajectory.offer_states, at most n_states); from each, for its own lowest-numbered
        candidate, gate_audit runs `replicates` pairs of a forced-enter and a forced-decline episode, replicate r with the seed
        `seed` + r (so with its own draws); the target is Delta(s) = mean G_enter - mean G_decline over the replicates (float64). Per
        option k with at least `min_offers` fit states, u_k is the ridge regression of Delta on the 1296 features: the audited
        states of even position are the fit half, the odd ones are held out; ONE ScgContext.feature_gram call with the option as
        the segment, then valuefit.ridge_solve. Returns (report, u): u {k: float64 [1296]}; report["options"] one row per offered
        option with "option", "n" (its audited states), "n_fit", "n_held", "fitted" and, on the held-out half, "rmse" (of float32
        u_k . phi against Delta, NaN where not fitted), "agreement_fitted" (sign(u_k . phi) >= 0 against Delta >= 0),
        "agreement_shipped" (V_k >= V_0 against the same), "mean_delta"; report["n_states"], "replicates", "epsilon", "ridge". The
        later steps of every branch act under the agent's W and SPEC §4.2's own gate. The agent is left as evaluate() leaves it."""
        from .valuefit import ridge_solve
        R = int(replicates)
        if R < 1 or int(min_offers) < 1:
            raise ValueError("fit_gate needs replicates >= 1 and min_offers >= 1")
        base_seed = int(self.ctx.cfg.seed) if seed is None else int(seed)
        traj, _ = self.record_episodes(int(n_record), epsilon=epsilon, seed=seed)
        states = traj.offer_states(int(n_states))
        report = {"n_states": int(len(states[0])), "replicates": R, "epsilon": float(epsilon), "ridge": float(ridge), "options": []}
        if not len(states[0]):
            return report, {}
        per0, ge, gd = None, 0.0, 0.0
        for r in range(R):
            per = self.gate_audit(states=states, epsilon=epsilon, seed=base_seed + r)["per_state"]
            if per0 is None:
                per0 = per
            elif not np.array_equal(per["index"], per0["index"]) or not np.array_equal(per["option"], per0["option"]):
                raise ScgError("fit_gate: two replicates audited different states")       # (the candidate is the state's alone)
            ge, gd = ge + per["g_enter"].astype(np.float64), gd + per["g_decline"].astype(np.float64)
        delta = (ge - gd) / R
        idx, opt = per0["index"], per0["option"]
        ships = per0["v_k"] >= per0["v_0"]                     # §4.2's decision at these states (a NaN side declines)
        fit = np.arange(len(idx)) % 2 == 0
        dev = self.W.device
        ectx = self._eval_ctx[len(states[0])][0]
        st = [torch.from_numpy(np.ascontiguousarray(v[idx])).to(dev) for v in states]
        ks = [int(k) for k in np.unique(opt)]
        if not ks:                                             # no offer state has a candidate now
            return report, {}
        order = np.concatenate([np.nonzero(fit & (opt == k))[0] for k in ks])           # the fit half by option, state order within one
        n_k = np.asarray([int(np.sum(fit & (opt == k))) for k in ks], np.int64)
        u = {}
        if len(order):
            at = torch.from_numpy(order).to(dev)
            A, b = ectx.feature_gram([t[at].contiguous() for t in st], np.concatenate([[0], np.cumsum(n_k)]).astype(np.int64),
                                     torch.from_numpy(delta[order].astype(np.float32)).to(dev))
            use = [i for i, k in enumerate(ks) if n_k[i] >= int(min_offers)]
            if use:
                sol = ridge_solve(A[use].cpu().numpy(), b[use].cpu().numpy(), n_k[use], ridge, self.ctx.scale)
                u = {ks[i]: sol[j] for j, i in enumerate(use)}
        nan = float("nan")
        for i, k in enumerate(ks):
            held = np.nonzero(~fit & (opt == k))[0]
            row = {"option": k, "n": int(np.sum(opt == k)), "n_fit": int(n_k[i]), "n_held": int(len(held)), "fitted": k in u,
                   "rmse": nan, "agreement_fitted": nan, "agreement_shipped": nan, "mean_delta": nan}
            if len(held):
                want = delta[held] >= 0.0
                row["agreement_shipped"] = float(np.mean(ships[held] == want))
                row["mean_delta"] = float(np.mean(delta[held]))
                if k in u:
                    Wk = torch.from_numpy(np.tile(u[k].astype(np.float32), (NUM_ACTIONS, 1))).to(dev).contiguous().view(-1)
                    pred = np.zeros(len(held), np.float32)
                    for j in range(0, len(held), ectx.n_envs):
                        sl = torch.from_numpy(held[j:j + ectx.n_envs]).to(dev)
                        pred[j:j + ectx.n_envs] = ectx.q_values([t[sl].contiguous() for t in st], Wk)[0].cpu().numpy()
                    row["rmse"] = float(np.sqrt(np.mean((pred.astype(np.float64) - delta[held]) ** 2)))
                    row["agreement_fitted"] = float(np.mean((pred >= 0.0) == want))
            report["options"].append(row)
        return report, u

    def improve_gate(self, eval_epsilons=(0.0,), criterion: str = "discounted", z: float = 2.0, n_eval: int = 4096,
                     apply: bool = False, **fit):
        """A safeguarded step on the value gate itself (SPEC §25.3), the counterpart of improve_policy for W and of
        improve_initiation for in_k. fit_gate(**fit) gives u; gatefit.candidate_gates(W, u) — SPEC §4.2's own comparison
        ("shipped"), "always", "never", each fitted option's row alone, and "all" — at each of `eval_epsilons` are evaluated in ONE
        evaluate_policies run of n_eval episodes each under the agent's W and clf (common start states and draws);
        initfit.choose_table decides at eval_epsilons[0] against "shipped" (SPEC §21.4's rule). Returns (report, gate_chosen):
        report["fit"] the fit's report, report["candidates"] rows of {"label", "epsilon", "summary", "paired"} (paired: against
        "shipped" at the same epsilon; the summary holds SPEC §8's per-option entries, declines and steps_share), "chosen" (a
        label; "shipped" when nothing is accepted), "accepted", "criterion", "z"; gate_chosen a copy of the chosen table.
        apply=True stores it as the agent's `gate`, under which evaluate() and evaluate_policies() then act by default (a copy:
        the "shipped" table is W's comparison as W was then; set `gate = None` to follow W again). ONLY those two read it: the learner (step_batch), option trials, branch and audit
        rollouts, the recorded evaluation and every other kernel keep SPEC §4.2's comparison under W. apply=True is refused on a
        sharded agent. ValueError for no epsilon, an unknown criterion, or more candidates x epsilons than a population holds.
        With apply=False the agent is left as evaluate() leaves it."""
        from . import gatefit
        if apply and self.group is not None:
            raise ValueError("improve_gate(apply=True) is not available on a sharded agent")
        if criterion not in ("discounted", "return", "success"):
            raise ValueError(f"criterion must be 'discounted', 'return' or 'success', not {criterion!r}")
        eps = [float(v) for v in eval_epsilons]
        if not eps:
            raise ValueError("improve_gate needs at least one epsilon")
        n_opt = bin(self.enabled_mask >> 1).count("1")
        if (3 + n_opt + (1 if n_opt >= 2 else 0)) * len(eps) > _lib.POP_MAX:          # before anything runs: the most the fit can give
            raise ValueError(f"{3 + n_opt + (1 if n_opt >= 2 else 0)} candidate gates x {len(eps)} epsilons are more than the "
                             f"{_lib.POP_MAX} policies of one population")
        fit_report, u = self.fit_gate(**fit)
        tables = gatefit.candidate_gates(self.W, u)
        n_tab, per_eps = len(tables), len(eps)
        stack = torch.stack([t for _, t in tables])
        summaries, _, envs = self.evaluate_policies(self.W, np.repeat(np.asarray(eps, np.float32), n_tab), None, n_episodes=int(n_eval),
                                                    seed=fit.get("seed"), per_env=True, gate=stack.repeat(per_eps, 1, 1, 1, 1))
        cands = [{"label": tables[i][0], "epsilon": eps[e], "summary": summaries[e * n_tab + i],
                  "paired": paired_differences(envs[e * n_tab + i], envs[e * n_tab])} for e in range(per_eps) for i in range(n_tab)]
        pick = initfit.choose_table(cands[:n_tab], criterion, z)
        gate_chosen = dict(tables)[pick["chosen"]].clone()
        if apply:
            self.gate = gate_chosen
        return {"fit": fit_report, "candidates": cands, "chosen": pick["chosen"], "accepted": pick["accepted"],
                "criterion": criterion, "z": float(z)}, gate_chosen

    def rollout(self, steps: int, learn: bool = True) -> None:
        for _ in range(steps):
            self.step_batch(learn)

