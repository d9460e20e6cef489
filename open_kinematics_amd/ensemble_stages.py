"""
The stages ``dist.ShardedEnsemble(reduce=True)`` runs over every rank's own shard of an evaluated ensemble: ``Reduction``
(moments, extremes, sensitivities), ``Sobol`` (``sobol=True``), ``SobolBootstrap`` (``bootstrap=``), ``Selection`` (``quantiles=``), ``Screening`` (``screen=True``), ``Covariance``
(``covariance=``), ``Effects`` (``effects=``), ``WhatIf`` (``whatif=``), ``Surface`` (``surface=``), ``Curves`` (``curves=``) and ``Front`` (``front=``).  One protocol, which ``ShardedEnsemble`` drives over the stages that are switched on, in this order:

* the constructor takes the owning ensemble and the stage's own arguments: it validates, allocates and sets ``bytes_per_rank``;
* ``begin_step()``; ``rows(a, b, local)``: geometries ``[a, b)`` of this rank (rows ``local`` of its tables) are taken in - the
  first chunk of a step writes, later chunks accumulate;
* ``end_step()``: a rank that took in nothing contributes the neutral element (the pass over no geometry), then the stage's
  collectives run - on every rank, whether or not it holds a geometry; then the result accessors answer.

A stage runs the device pass (``ensemble_device.py``) when the ensemble lives on a GPU and the NumPy stand-in of
``ensemble_stats.py`` otherwise (the CPU tests): decided once, and never a quiet host pass over device tables.
"""

from __future__ import annotations

import numpy as np
import torch

from . import ensemble_stats as es
from .dist import all_gather_flat, all_reduce_sum, broadcast_from_rank_zero


class _Stage:
    bytes_per_rank = 0

    def __init__(self, owner):
        self.owner = owner
        self.on_device = owner.device.type == "cuda"
        self.taken = False  # something was taken in since begin_step()

    def begin_step(self) -> None:
        self.taken = False

    def rows(self, a: int, b: int, local) -> None:
        o = self.owner
        self.take(a, b, o.metric_local[local], o.info_local[local][:, 32])
        self.taken = True

    def end_step(self) -> None:
        if not self.taken:  # a rank without a geometry: the pass over no geometry, the neutral element
            glo = self.owner.geometry_range[0]
            self.rows(glo, glo, slice(0, 0))
        self.exchange()

    def host_tables(self, a: int, b: int, values, status) -> tuple:
        """``values [G', S, K]`` and ``status [G', S]`` of a chunk as the NumPy stand-ins take them."""
        steps = self.owner.steps
        return values.reshape(b - a, steps, values.shape[1]).cpu().numpy(), status.reshape(b - a, steps).cpu().numpy()


class _AccumulatorStage(_Stage):
    """A stage whose partial result is float64 tables that merge: packed, all-gathered, merged in rank order."""

    def allocate_exchange(self, words: int) -> None:
        o = self.owner
        self.send = torch.empty(words, dtype=torch.float64, device=o.device) if o.world > 1 else None
        self.recv = torch.empty((o.world, words), dtype=torch.float64, device=o.device) if o.world > 1 else None
        self.bytes_per_rank = 8 * words if o.world > 1 else 0

    def merged_over_ranks(self, mine, parts, unpack):
        """ONE all-gather of ``parts`` (this rank's tables, flat, in order) and the merge of ``unpack(row)`` of every rank's
        row in rank order: the same bits on every rank.  A world of one keeps ``mine``."""
        o = self.owner
        if o.world == 1:
            return mine
        at = 0
        for part in parts:
            self.send[at : at + part.numel()] = part.reshape(-1)
            at += part.numel()
        all_gather_flat(self.send, o.group, out=self.recv)
        merged = None
        for r in range(o.world):
            part = unpack(self.recv[r])
            merged = part if merged is None else merged.merge(part)
        return merged


class Reduction(_AccumulatorStage):
    """``reduce=True``: the accumulators of ``ensemble_stats.py`` instead of a gathered table."""

    def __init__(self, owner, hardpoints, targets, relative_targets, factors, shift):
        super().__init__(owner)
        o = owner
        glo, ghi = o.geometry_range
        device, k = o.device, len(o.metric_index)
        self.factor_names = None
        plan = getattr(o, "plan", None)
        self._all_factors = None
        if isinstance(factors, str) and factors == "sampled":
            # the plan's latents ARE the factors: the owner drew this rank's rows of them beside the rows it rebound, and they stay
            # where they are (one host copy for the moments below); a stage that reduces rows of every rank draws the whole table
            # when it asks for it (all_factors)
            mine = o.sampled_latents.contiguous()
            factors = mine.detach().cpu().numpy()
            self.factor_names = plan.factor_names()
            self._sampled = hardpoints
            if glo == 0 and ghi == o.n_geom:
                self._all_factors = factors
            self._finish(o, hardpoints, targets, relative_targets, factors, shift, glo, ghi, 0, mine)
            return
        if isinstance(factors, str):
            if factors != "hardpoints":
                raise ValueError("factors must be None, 'hardpoints', 'sampled' (with a SamplePlan) or a [G, P] table")
            program = o.dp.program
            if plan is not None:
                hardpoints = hardpoints[0 : o.n_geom]
            table = torch.as_tensor(hardpoints).detach().cpu().numpy()
            # (derived points are recomputed from the authored ones by rebind: their coordinates are no factors)
            from .program import key_name

            authored = np.setdiff1d(np.arange(table.shape[1]), np.asarray(program.dop_out, dtype=np.int64))
            names = [key_name(program.point_keys[i]).lower() for i in authored]
            factors, self.factor_names = es.hardpoint_factors(table[:, authored], names)
        if factors is not None:
            factors = np.ascontiguousarray(torch.as_tensor(factors).detach().cpu().numpy(), dtype=np.float64).reshape(o.n_geom, -1)
        self._all_factors = factors  # [G, P] on the host (or None): a stage that reduces rows of every rank takes them from here
        self._finish(o, hardpoints, targets, relative_targets, factors, shift, glo, ghi, glo)

    @property
    def all_factors(self):
        """``[G, P]`` on the host (or None): the factors of EVERY geometry, for a stage that reduces rows of every rank."""
        if self._all_factors is None and self.n_factors and getattr(self, "_sampled", None) is not None:
            self._all_factors = self._sampled.draw(0, self.owner.n_geom, latents=True)[1].detach().cpu().numpy()
        return self._all_factors

    def _finish(self, o, hardpoints, targets, relative_targets, factors, shift, glo, ghi, row0, resident=None):
        """The rest of the set-up; ``factors [*, P]`` on the host hold this rank's rows from row ``row0`` on (``resident``: the same
        rows already on the ensemble's device)."""
        device, k = o.device, len(o.metric_index)
        if factors is not None:
            factors = np.ascontiguousarray(factors, dtype=np.float64)[row0 : row0 + ghi - glo]
        p = 0 if factors is None else factors.shape[1]
        self.n_factors = p
        self.my_factors = (resident if resident is not None else torch.as_tensor(factors, device=device).contiguous()) if p else None
        # the shift: ONE table for every partial that is ever merged
        if shift is None:
            shift = torch.zeros((o.steps, k), dtype=torch.float64, device=device)
            if o.rank == 0 and o.n_geom > 0:
                gpos, gparam = o.dp.rebind(hardpoints[:1] if getattr(o, "plan", None) is not None else torch.as_tensor(hardpoints)[:1])
                first = o.dp.ensemble_targets(gpos, targets) if relative_targets else targets[: o.steps]
                res = o.dp.solve_evaluated(first, geom_pos=gpos, geom_row_param=gparam, steps_per_geometry=o.steps,
                                           output="none", **o.solve_kw)
                rows = res.eval.reshape(o.steps, -1).to(device)
                shift = torch.nan_to_num(torch.index_select(rows, 1, o.metric_index), nan=0.0, posinf=0.0, neginf=0.0)
            if o.world > 1:
                shift = broadcast_from_rank_zero(shift.contiguous(), o.group)
        else:
            shift = torch.as_tensor(es.clean_shift(torch.as_tensor(shift).detach().cpu().numpy()), device=device)
        shift = shift.reshape(o.steps, k).contiguous()
        # the unmasked factor moments of this rank's geometries, once: the factors never change (ascending order, as the device sums)
        factor_acc = None
        if p:
            mine = factors
            rows, cols = np.tril_indices(p)
            moments = np.zeros(es.factor_moment_count(p))
            if ghi > glo:
                moments[:p] = np.cumsum(mine, axis=0)[-1]
                moments[p:-1] = np.cumsum(mine[:, rows] * mine[:, cols], axis=0)[-1]
            moments[-1] = ghi - glo
            factor_acc = torch.as_tensor(moments, device=device)
        self.local = es.EnsembleAccumulator(torch.empty((o.steps, k, es.ENS_FIELDS + p), dtype=torch.float64, device=device),
                                            shift, factor_acc, self.factor_names)
        self.merged = self.local
        self.allocate_exchange(self.local.acc.numel() + (factor_acc.numel() if p else 0))

    def take(self, a: int, b: int, values, status) -> None:
        o, acc = self.owner, self.local
        glo = o.geometry_range[0]
        factors = self.my_factors[a - glo : b - glo] if self.n_factors else None
        if self.on_device:
            o.dp.reduce_ensemble(values, steps_per_geometry=o.steps, status=status, factors=factors, geometry_offset=a, out=acc,
                                 accumulate=self.taken, factor_moments=False)
            return
        part = es.reduce_host(*self.host_tables(a, b, values, status), None if factors is None else factors.cpu().numpy(), acc.shift.cpu().numpy(), a)
        part = es.EnsembleAccumulator(torch.as_tensor(part.acc, device=o.device), acc.shift, None)
        if self.taken:
            part = es.EnsembleAccumulator(acc.acc, acc.shift, None).merge(part)
        acc.acc.copy_(part.acc)

    def exchange(self) -> None:
        mine = self.local
        n_acc = mine.acc.numel()

        def unpack(row):
            return es.EnsembleAccumulator(row[:n_acc].reshape(mine.acc.shape), mine.shift, row[n_acc:] if self.n_factors else None, self.factor_names)

        self.merged = self.merged_over_ranks(mine, (mine.acc, mine.factor_acc) if self.n_factors else (mine.acc,), unpack)


class Sobol(_AccumulatorStage):
    """``sobol=True`` (the ensemble is a ``FamilyPlan``'s): the Sobol' accumulators, chunk by chunk right after the reduction, with the
    reduction's shift and the chunk's sampler flags as the mask; chunks and shards are whole families (``ShardedEnsemble.align``)."""

    def __init__(self, owner):
        super().__init__(owner)
        o = owner
        k, d = len(o.metric_index), o.plan.n_groups
        self.n_groups, self.group_names = d, o.plan.names()
        shift = o.local_accumulator.shift  # ONE table for every partial that is ever merged: the reduction's (itself, no copy)
        self.flags = o.sampled_flags.contiguous()
        self.local = es.SobolAccumulator(torch.zeros((o.steps, k, es.SOBOL_FIELDS + 3 * d), dtype=torch.float64, device=o.device), shift, self.group_names)
        self.merged = self.result = None
        self.allocate_exchange(self.local.acc.numel())

    def take(self, a: int, b: int, values, status) -> None:
        o, mine = self.owner, self.local
        glo = o.geometry_range[0]
        mask = self.flags[a - glo : b - glo]
        if self.on_device:
            o.dp.sobol_ensemble(values, steps_per_geometry=o.steps, n_groups=self.n_groups, status=status, mask=mask, out=mine, accumulate=self.taken)
            return
        part = es.sobol_host(*self.host_tables(a, b, values, status), mask.cpu().numpy(), self.n_groups, mine.shift.cpu().numpy())
        if not self.taken:
            mine.acc.zero_()
        mine.acc += torch.from_numpy(part.acc)

    def exchange(self) -> None:
        mine = self.local
        self.result = None
        self.merged = self.merged_over_ranks(mine, (mine.acc,), lambda row: es.SobolAccumulator(row.reshape(mine.acc.shape), mine.shift, self.group_names))

    def sobol(self):
        if self.merged is None:
            raise RuntimeError("no step() yet")
        if self.result is None:
            self.result = self.merged.finalize()
        return self.result


class SobolBootstrap(_AccumulatorStage):
    """``sobol=True, bootstrap=R``: ``R`` Poisson-bootstrap replicates of the Sobol' accumulators, each chunk right after the Sobol' stage
    took it, with the same shift and mask; the chunk's first family ``a // family_size`` is its ``family_offset``, so the replicates do
    not depend on how the ensemble is sharded or chunked."""

    def __init__(self, owner, n_replicates: int, seed: int):
        super().__init__(owner)
        o = owner
        k, d = len(o.metric_index), o.plan.n_groups
        self.n_groups, self.group_names, self.family_size = d, o.plan.names(), o.plan.family_size
        self.n_replicates, self.seed = es.check_replicates("bootstrap=", n_replicates), int(seed) & 0xFFFFFFFFFFFFFFFF
        sobol = o.stages["sobol"]
        self.flags = sobol.flags
        self.local = es.SobolBootstrapAccumulator(torch.zeros((self.n_replicates, o.steps, k, es.SOBOL_FIELDS + 3 * d), dtype=torch.float64, device=o.device),
                                                  sobol.local.shift, self.seed, self.group_names)  # ONE shift: the reduction's (itself, no copy)
        self.merged = self.result = None
        self.allocate_exchange(self.local.acc.numel())

    def take(self, a: int, b: int, values, status) -> None:
        o, mine = self.owner, self.local
        glo = o.geometry_range[0]
        mask = self.flags[a - glo : b - glo]
        first = a // self.family_size
        if self.on_device:
            o.dp.sobol_bootstrap_ensemble(values, steps_per_geometry=o.steps, n_groups=self.n_groups, n_replicates=self.n_replicates, seed=self.seed,
                                          family_offset=first, status=status, mask=mask, out=mine, accumulate=self.taken)
            return
        part = es.sobol_bootstrap_host(*self.host_tables(a, b, values, status), mask.cpu().numpy(), self.n_groups, mine.shift.cpu().numpy(),
                                       seed=self.seed, n_replicates=self.n_replicates, family_offset=first)
        if not self.taken:
            mine.acc.zero_()
        mine.acc += torch.from_numpy(part.acc)

    def exchange(self) -> None:
        mine = self.local
        self.result = None
        self.merged = self.merged_over_ranks(mine, (mine.acc,), lambda row: es.SobolBootstrapAccumulator(row.reshape(mine.acc.shape), mine.shift, self.seed,
                                                                                                        self.group_names))

    def sobol_bootstrap(self, level: float = 0.95):
        if self.merged is None:
            raise RuntimeError("no step() yet")
        if self.result is None or self.result.level != float(level):
            self.result = self.merged.finalize(level)
        return self.result


class Selection(_Stage):
    """``quantiles=...``: the select rounds over the rank's whole shard at the end of a step, the histograms summed over the ranks."""

    def __init__(self, owner, quantiles, limits):
        super().__init__(owner)
        o = owner
        k = len(o.metric_index)
        self.probs, self.limits = es.check_select_arguments(quantiles, limits, o.steps, k)
        self.run = self.result = None
        self.stepped = False
        if self.on_device:
            self.run = o.dp.select_prepare(o.steps, k, self.probs, self.limits, rounds=True)
            rounds, words = o.dp.select_rounds, self.run.hist.numel()
        else:
            rounds, words = es.SELECT_ROUNDS, o.steps * k * 2 * len(self.probs) * es.SELECT_BINS
        self.bytes_per_rank = rounds * 8 * words if o.world > 1 else 0

    def rows(self, a: int, b: int, local) -> None:
        pass

    def end_step(self) -> None:
        """Every round: count this rank's shard, sum the histograms over the ranks (one all-reduce), descend."""
        o = self.owner
        glo, ghi = o.geometry_range
        values, status = o.metric_local, o.info_local[:, 32]
        if self.on_device:
            run, dp = self.run, o.dp
            dp.select_begin(run)
            for rnd in range(dp.select_rounds):
                if ghi > glo:  # (a rank without a geometry contributes a zero histogram)
                    dp.select_count(run, rnd, values, steps_per_geometry=o.steps, status=status)
                all_reduce_sum(run.hist, o.group)
                dp.select_descend(run, rnd)
            dp.select_finish(run)
            self.result, self.stepped = None, True
            return
        v, st = self.host_tables(glo, ghi, values, status)
        state, hist = es.select_begin(o.steps, values.shape[1], len(self.probs))
        for rnd in range(es.SELECT_ROUNDS):
            es.select_count_round(rnd, v, st, state, hist, self.limits)
            all_reduce_sum(torch.from_numpy(hist), o.group)
            es.select_descend_round(rnd, state, hist, self.probs)
        self.result = es.select_finish(state, self.probs, self.limits is not None)

    def quantiles(self):
        if self.result is None:
            if not self.stepped:
                raise RuntimeError("no step() yet")
            self.result = self.run.finalize()
        return self.result


class Screening(_Stage):
    """``screen=True``: the joint verdict per geometry, chunk by chunk; ``tally | blame`` summed and the flag bytes gathered."""

    def __init__(self, owner, limits, scale):
        super().__init__(owner)
        o = owner
        glo, ghi = o.geometry_range
        k = len(o.metric_index)
        self.limits, self.scale = es.check_screen_arguments(limits, scale, o.steps, k)
        self.largest_shard = max(hi - lo for lo, hi in (o.shard_of(r) for r in range(o.world)))
        self.run = self.part = self.result = self.counts = self.flags = None
        if self.on_device:
            self.run = o.dp.screen_prepare(o.steps, k, self.limits, self.scale, ghi - glo)
        self.bytes_per_rank = 8 * (4 + 2 * o.steps * k) + self.largest_shard if o.world > 1 else 0

    def take(self, a: int, b: int, values, status) -> None:
        o = self.owner
        if self.on_device:
            o.dp.screen_ensemble(values, steps_per_geometry=o.steps, status=status, geometry_offset=a, out=self.run,
                                 accumulate=self.taken, first_row=a - o.geometry_range[0])
            return
        part = es.screen_host(*self.host_tables(a, b, values, status), self.limits, self.scale, a)
        self.part = self.part.merge(part) if self.taken else part

    def exchange(self) -> None:
        """One integer all-reduce of tally | blame and one all-gather of the flag bytes (padded to the largest shard): the same
        bits on every rank."""
        o = self.owner
        if self.on_device:
            counts, flags = torch.cat([self.run.tally, self.run.blame.reshape(-1)]), self.run.flags
        else:
            counts, flags = torch.from_numpy(np.concatenate([self.part.tally, self.part.blame.reshape(-1)])), torch.from_numpy(self.part.flags)
        self.result = None
        if o.world > 1:
            padded = torch.zeros(self.largest_shard, dtype=torch.uint8, device=flags.device)
            padded[: flags.shape[0]] = flags
            all_reduce_sum(counts, o.group)
            table = all_gather_flat(padded, o.group)
            spans = [o.shard_of(r) for r in range(o.world)]
            flags = torch.cat([table[r, : hi - lo] for r, (lo, hi) in enumerate(spans)])
        self.counts, self.flags = counts, flags

    def screen(self):
        if self.counts is None:
            raise RuntimeError("no step() yet")
        if self.result is None:
            o = self.owner
            counts, flags = self.counts.cpu().numpy(), self.flags.cpu().numpy()
            blame = counts[4:].reshape(o.steps, len(o.metric_index), 2).copy()
            self.result = es.EnsembleScreen(flags, None, None, counts[:4].copy(), blame, np.flatnonzero(flags == 0).astype(np.int64))
        return self.result

    def screen_local(self) -> dict:
        if self.on_device:
            run = self.run
            return {"flags": run.flags, "margin": run.margin, "entry": run.entry, "pass_index": run.pass_index, "pass_count": run.pass_count}
        if self.part is None:
            raise RuntimeError("no step() yet")
        part = self.part
        return {"flags": torch.from_numpy(part.flags), "margin": torch.from_numpy(part.margin), "entry": torch.from_numpy(part.entry),
                "pass_index": torch.from_numpy(part.passed), "pass_count": torch.tensor([part.passed.size], dtype=torch.int64)}


class Covariance(_AccumulatorStage):
    """``covariance=...``: Gram matrix, sums and counts of the selected entries, chunk by chunk, with the reduction's shift."""

    def __init__(self, owner, covariance):
        super().__init__(owner)
        o = owner
        glo, ghi = o.geometry_range
        k, device = len(o.metric_index), o.device
        entries = es.check_covariance_arguments(None if covariance is True else
                                                (covariance.detach().cpu().numpy() if isinstance(covariance, torch.Tensor) else covariance), o.steps * k)
        n = int(entries.size)
        self.entries = entries
        shift = o.local_accumulator.shift  # ONE table for every partial that is ever merged: the reduction's (itself, no copy)
        self.local = es.CovarianceAccumulator(torch.zeros((n, n), dtype=torch.float64, device=device), torch.zeros(n, dtype=torch.float64, device=device),
                                              torch.zeros(2, dtype=torch.int64, device=device), shift, torch.as_tensor(entries, device=device),
                                              torch.zeros(ghi - glo, dtype=torch.uint8, device=device), natural=covariance is True)
        self.merged = self.result = None
        self.allocate_exchange(n * n + n + 2)

    def take(self, a: int, b: int, values, status) -> None:
        o, mine = self.owner, self.local
        glo = o.geometry_range[0]
        if self.on_device:
            view = es.CovarianceAccumulator(mine.gram, mine.sum, mine.counts, mine.shift, mine.entries, mine.used[a - glo :], natural=mine.natural)
            o.dp.covariance_ensemble(values, steps_per_geometry=o.steps, status=status, out=view, accumulate=self.taken)
            return
        part = es.covariance_host(*self.host_tables(a, b, values, status), self.entries, mine.shift.cpu().numpy())
        if not self.taken:
            mine.gram.zero_(), mine.sum.zero_(), mine.counts.zero_()
        mine.gram += torch.from_numpy(part.gram)
        mine.sum += torch.from_numpy(part.sum)
        mine.counts += torch.from_numpy(part.counts)
        mine.used[a - glo : b - glo] = torch.from_numpy(part.used)

    def exchange(self) -> None:
        """(the counts travel as their int64 bits)"""
        mine = self.local
        n = int(mine.entries.shape[0])
        self.result = None

        def unpack(row):
            return es.CovarianceAccumulator(row[: n * n].reshape(n, n), row[n * n : n * n + n], row[n * n + n :].view(torch.int64), mine.shift, mine.entries)

        self.merged = self.merged_over_ranks(mine, (mine.gram, mine.sum, mine.counts.view(torch.float64)), unpack)

    def covariance(self):
        if self.merged is None:
            raise RuntimeError("no step() yet")
        if self.result is None:
            self.result = self.merged.finalize()
        return self.result


class Effects(_AccumulatorStage):
    """``effects=n_bins`` or ``effects=dict(bins=, edges=)``: the conditional moments of every entry over equal-probability bins of each of
    the reduction's factors, chunk by chunk right after the reduction, with the reduction's shift and - when the ensemble was sampled -
    the sampler's flag bytes as the mask.  The edges are the same bits on every rank: analytic from the plan for ``factors="sampled"``,
    else the order statistics of the factors of ALL geometries.  A chunk's factor rows are binned once, the first time it is taken in:
    factors do not change from step to step."""

    def __init__(self, owner, effects):
        super().__init__(owner)
        o = owner
        reduction = o.stages["reduce"]
        edges = None
        if isinstance(effects, dict):
            unknown = set(effects) - {"bins", "edges"}
            if unknown or "bins" not in effects:
                raise ValueError(f"effects= takes an integer or dict(bins=, edges=) (got {sorted(effects)})")
            effects, edges = effects["bins"], effects.get("edges")
        p = reduction.n_factors
        if not p:
            raise ValueError("effects= bins the reduction's factors: it needs factors=")
        n_bins = es.check_effects_arguments(effects, p)[0]
        if edges is None:
            if getattr(reduction, "_sampled", None) is not None:
                edges = es.effects_edges(getattr(o.plan, "plan", o.plan), n_bins)  # (a FamilyPlan wraps the plan its rows are drawn from)
            else:
                edges = es.effects_edges(reduction.all_factors, n_bins)
        elif isinstance(edges, torch.Tensor):
            edges = edges.detach().cpu().numpy()
        self.n_bins, self.edges, _ = es.check_effects_arguments(n_bins, p, edges)
        self.factor_names = reduction.factor_names
        self.factors = reduction.my_factors  # this rank's rows [n, P], where the ensemble lives
        self.flags = o.sampled_flags.contiguous() if o.sampled_flags is not None else None
        k = len(o.metric_index)
        shift = o.local_accumulator.shift  # ONE table for every partial that is ever merged: the reduction's (itself, no copy)
        self.local = es.EffectsAccumulator(torch.zeros((p, self.n_bins, es.EFFECTS_FIELDS, o.steps, k), dtype=torch.float64, device=o.device), shift,
                                           torch.as_tensor(self.edges, device=o.device), self.factor_names)
        self.binned = {}  # (a, b) -> the bins of the chunk's rows
        self.merged = self.result = None
        self.allocate_exchange(self.local.acc.numel())

    def take(self, a: int, b: int, values, status) -> None:
        o, mine = self.owner, self.local
        glo = o.geometry_range[0]
        mask = None if self.flags is None else self.flags[a - glo : b - glo]
        bins = self.binned.get((a, b))
        if self.on_device:
            if bins is None:
                bins = self.binned[(a, b)] = o.dp.bin_factors(self.factors[a - glo : b - glo], self.edges)
            o.dp.effects_ensemble(values, steps_per_geometry=o.steps, bins=bins, status=status, mask=mask, out=mine, accumulate=self.taken)
            return
        if bins is None:
            bins = self.binned[(a, b)] = es.bin_factors_host(self.factors[a - glo : b - glo].cpu().numpy(), self.edges)
        part = es.effects_host(*self.host_tables(a, b, values, status), None if mask is None else mask.cpu().numpy(), bins, self.n_bins,
                               mine.shift.cpu().numpy(), self.edges)
        if not self.taken:
            mine.acc.zero_()
        mine.acc += torch.from_numpy(part.acc)

    def exchange(self) -> None:
        mine = self.local
        self.result = None
        self.merged = self.merged_over_ranks(mine, (mine.acc,), lambda row: es.EffectsAccumulator(row.reshape(mine.acc.shape), mine.shift, mine.edges,
                                                                                                  self.factor_names))

    def effects(self):
        if self.merged is None:
            raise RuntimeError("no step() yet")
        if self.result is None:
            self.result = self.merged.finalize()
        return self.result


class WhatIf(_AccumulatorStage):
    """``whatif=scenarios`` (with ``factors="sampled"``): what every entry's scatter and yield become under each tolerance scenario, chunk
    by chunk right after the reduction (and the screen), with the reduction's shift, the sampler's flag bytes as the mask, ``limits=``
    when given and - with ``screen=True`` - the screen's flag bytes as the verdict.  ``scenarios`` is the list of specs
    ``ensemble_sample.tolerance_scenarios`` takes, or the table it returns.  A chunk's weights are computed once, the first time it is
    taken in: latents do not change from step to step."""

    def __init__(self, owner, whatif, limits):
        super().__init__(owner)
        from .ensemble_sample import check_tilt, tolerance_scenarios

        o = owner
        reduction = o.stages["reduce"]
        if isinstance(whatif, (np.ndarray, torch.Tensor)):
            whatif = whatif.detach().cpu().numpy() if isinstance(whatif, torch.Tensor) else whatif
            self.tilt = check_tilt(whatif)
            if self.tilt.shape[1] != o.plan.n_latents:
                raise ValueError(f"whatif=: the scenario table has {self.tilt.shape[1]} latents, the plan {o.plan.n_latents}")
        else:
            self.tilt = tolerance_scenarios(o.plan, whatif)
        n, k = int(self.tilt.shape[0]), len(o.metric_index)
        self.limits = None if limits is None else es.check_reweigh_limits(limits, o.steps, k)
        self.latents = reduction.my_factors  # this rank's rows [n, Z] of the plan's latents, where the ensemble lives
        self.flags = o.sampled_flags.contiguous()
        shift = o.local_accumulator.shift  # ONE table for every partial that is ever merged: the reduction's (itself, no copy)
        self.local = es.ReweighAccumulator(torch.zeros((n, es.REWEIGH_FIELDS, o.steps, k), dtype=torch.float64, device=o.device),
                                           torch.zeros((n, es.REWEIGH_JOINT_FIELDS), dtype=torch.float64, device=o.device), shift,
                                           None if self.limits is None else torch.as_tensor(self.limits, device=o.device))
        self.table = o.dp.tilt_prepare(self.tilt) if self.on_device else None
        self.weights = {}  # (a, b) -> the weights of the chunk's rows
        self.merged = self.result = None
        self.allocate_exchange(self.local.acc.numel() + self.local.joint.numel())

    def take(self, a: int, b: int, values, status) -> None:
        from .ensemble_sample import tilt_weights_host

        o, mine = self.owner, self.local
        glo = o.geometry_range[0]
        rows = slice(a - glo, b - glo)
        mask, weights, verdict = self.flags[rows], self.weights.get((a, b)), None
        screen = o.stages.get("screen")
        if self.on_device:
            if weights is None:
                weights = self.weights[(a, b)] = o.dp.tilt_weights(self.latents[rows], self.table)
            if screen is not None:
                verdict = screen.run.flags[rows]
            o.dp.reweigh_ensemble(values, steps_per_geometry=o.steps, weights=weights, status=status, mask=mask, verdict=verdict, out=mine,
                                  accumulate=self.taken)
            return
        if weights is None:
            weights = self.weights[(a, b)] = tilt_weights_host(self.latents[rows].cpu().numpy(), self.tilt)
        if screen is not None:
            verdict = np.ascontiguousarray(screen.part.flags[rows])
        part = es.reweigh_host(*self.host_tables(a, b, values, status), mask.cpu().numpy(), weights, mine.shift.cpu().numpy(), self.limits, verdict)
        if not self.taken:
            mine.acc.zero_(), mine.joint.zero_()
        mine.acc += torch.from_numpy(part.acc)
        mine.joint += torch.from_numpy(part.joint)

    def exchange(self) -> None:
        mine = self.local
        n_acc = mine.acc.numel()
        self.result = None

        def unpack(row):
            return es.ReweighAccumulator(row[:n_acc].reshape(mine.acc.shape), row[n_acc:].reshape(mine.joint.shape), mine.shift, mine.limits)

        self.merged = self.merged_over_ranks(mine, (mine.acc, mine.joint), unpack)

    def whatif(self):
        if self.merged is None:
            raise RuntimeError("no step() yet")
        if self.result is None:
            self.result = self.merged.finalize()
        return self.result


class Surface(_AccumulatorStage):
    """``surface=True`` or ``surface=dict(degree=, interactions=, entries=, factors=)``: the normal equations of a polynomial response surface
    of the selected entries on the reduction's factors, chunk by chunk right after the reduction, with the reduction's shift and - when the
    ensemble was sampled - the sampler's flag bytes as the mask.  The basis is the same bits on every rank: from the plan's laws for
    ``factors="sampled"``, else from the factor table of ALL geometries.  A chunk's basis rows are built once, the first time it is taken
    in: factors do not change from step to step."""

    def __init__(self, owner, surface):
        super().__init__(owner)
        o = owner
        reduction = o.stages["reduce"]
        options = {} if surface is True else dict(surface)
        unknown = set(options) - {"degree", "interactions", "entries", "factors"}
        if unknown:
            raise ValueError(f"surface= takes True or dict(degree=, interactions=, entries=, factors=) (got {sorted(options)})")
        if not reduction.n_factors:
            raise ValueError("surface= regresses on the reduction's factors: it needs factors=")
        k, device = len(o.metric_index), o.device
        entries = options.get("entries")
        if entries is None and o.steps * k > es.SURFACE_MAX_ENTRIES:
            raise ValueError(f"surface=: the table has {o.steps * k} entries, more than {es.SURFACE_MAX_ENTRIES}: choose some with entries=")
        source = o.plan if getattr(reduction, "_sampled", None) is not None else reduction.all_factors
        self.basis = es.surface_terms(source, options.get("degree", 2), options.get("interactions", True), options.get("factors"))
        if self.basis.factor_names is None and reduction.factor_names is not None:
            self.basis.factor_names = tuple(reduction.factor_names)
        t = self.basis.n_terms
        self.entries = es.check_surface_arguments(entries.detach().cpu().numpy() if isinstance(entries, torch.Tensor) else entries, o.steps * k, t)
        n = int(self.entries.size)
        glo, ghi = o.geometry_range
        self.factors = reduction.my_factors  # this rank's rows [n, P], where the ensemble lives
        self.flags = o.sampled_flags.contiguous() if o.sampled_flags is not None else None
        shift = o.local_accumulator.shift  # ONE table for every partial that is ever merged: the reduction's (itself, no copy)
        self.local = es.SurfaceAccumulator(torch.zeros((t, t), dtype=torch.float64, device=device), torch.zeros((t, n), dtype=torch.float64, device=device),
                                           torch.zeros(n, dtype=torch.float64, device=device), torch.zeros(2, dtype=torch.int64, device=device), shift,
                                           torch.as_tensor(self.entries, device=device), torch.zeros(ghi - glo, dtype=torch.uint8, device=device),
                                           basis=self.basis, natural=entries is None)
        self.rows_of = {}  # (a, b) -> the basis rows of the chunk
        self.merged = self.result = None
        self.allocate_exchange(t * t + t * n + n + 2)

    def take(self, a: int, b: int, values, status) -> None:
        o, mine = self.owner, self.local
        glo = o.geometry_range[0]
        rows = slice(a - glo, b - glo)
        mask = None if self.flags is None else self.flags[rows]
        table = self.rows_of.get((a, b))
        if self.on_device:
            if table is None:
                table = self.rows_of[(a, b)] = o.dp.basis_factors(self.factors[rows], self.basis)
            view = es.SurfaceAccumulator(mine.gram, mine.cross, mine.sumsq, mine.counts, mine.shift, mine.entries, mine.used[a - glo :], basis=self.basis,
                                         natural=mine.natural)
            o.dp.surface_ensemble(values, steps_per_geometry=o.steps, basis_table=table, status=status, mask=mask, out=view, accumulate=self.taken)
            return
        if table is None:
            table = self.rows_of[(a, b)] = es.basis_host(self.factors[rows].cpu().numpy(), self.basis)
        part = es.surface_host(*self.host_tables(a, b, values, status), None if mask is None else mask.cpu().numpy(), table[0], table[1], self.entries,
                               mine.shift.cpu().numpy(), basis=self.basis)
        if not self.taken:
            mine.gram.zero_(), mine.cross.zero_(), mine.sumsq.zero_(), mine.counts.zero_()
        mine.gram += torch.from_numpy(part.gram)
        mine.cross += torch.from_numpy(part.cross)
        mine.sumsq += torch.from_numpy(part.sumsq)
        mine.counts += torch.from_numpy(part.counts)
        mine.used[rows] = torch.from_numpy(part.used)

    def exchange(self) -> None:
        """(the counts travel as their int64 bits)"""
        mine = self.local
        t, n = self.basis.n_terms, int(mine.entries.shape[0])
        self.result = None

        def unpack(row):
            at = (t * t, t * t + t * n, t * t + t * n + n)
            return es.SurfaceAccumulator(row[: at[0]].reshape(t, t), row[at[0] : at[1]].reshape(t, n), row[at[1] : at[2]], row[at[2] :].view(torch.int64),
                                         mine.shift, mine.entries, basis=self.basis)

        self.merged = self.merged_over_ranks(mine, (mine.gram, mine.cross, mine.sumsq, mine.counts.view(torch.float64)), unpack)

    def surface(self):
        if self.merged is None:
            raise RuntimeError("no step() yet")
        if self.result is None:
            self.result = self.merged.finalize()
        return self.result


class Curves(_Stage):
    """``curves=dict(abscissa=, origin=, scale=, degree=, window=)``: every geometry's curve characteristics along the sweep, chunk
    by chunk into this rank's feature table.  At the end of a step the ranks all-gather their feature rows (96 bytes per
    geometry and column - a table ``S / 12`` times smaller than the one it came from) and every rank reduces the SAME table
    ``[G, K * 12]``, one step per geometry, with the same factors and the same shift: the answer does not depend on how the
    geometries were sharded or chunked."""

    def __init__(self, owner, curves):
        super().__init__(owner)
        o = owner
        glo, ghi = o.geometry_range
        k, device = len(o.metric_index), o.device
        unknown = set(curves) - {"abscissa", "origin", "scale", "degree", "window"}
        if unknown or "abscissa" not in curves or "scale" not in curves:
            raise ValueError(f"curves= takes abscissa, scale and optionally origin, degree, window (got {sorted(curves)})")
        kw = dict(abscissa=curves["abscissa"], origin=curves.get("origin", 0.0), scale=curves["scale"], degree=curves.get("degree", 2),
                  window=curves.get("window"))
        self.arguments = es.check_curve_arguments(kw["abscissa"], kw["origin"], kw["scale"], kw["degree"], kw["window"], o.steps, k)
        self.host_kw = dict(kw, abscissa=kw["abscissa"] if self.arguments[0] is None else self.arguments[0])
        reduction = o.stages["reduce"]
        n = k * es.CURVE_FIELDS
        # the common shift: the features of the reduction's own shift table - the nominal geometry's rows, the same on every
        # rank, so nobody solves again
        if self.on_device:
            self.local = o.dp.curves_prepare(o.steps, k, ghi - glo, **self.host_kw)
            nominal = o.dp.curves_ensemble(reduction.local.shift, steps_per_geometry=o.steps, **self.host_kw)
            shift = torch.nan_to_num(nominal.table(), nan=0.0, posinf=0.0, neginf=0.0)
        else:
            self.local = es.EnsembleCurves(torch.full((ghi - glo, k, es.CURVE_FIELDS), float("nan"), dtype=torch.float64),
                                           torch.zeros((ghi - glo, k), dtype=torch.int32), None, self.arguments[1:])
            nominal = es.curves_host(reduction.local.shift.cpu().numpy()[None], None, **self.host_kw)
            shift = torch.as_tensor(es.clean_shift(nominal.table()))
        p = reduction.n_factors
        self.n_factors, self.factor_names = p, reduction.factor_names
        self.factors = torch.as_tensor(reduction.all_factors, device=device).contiguous() if p else None  # [G, P]: every rank reduces every row
        self.acc = es.EnsembleAccumulator(torch.empty((1, n, es.ENS_FIELDS + p), dtype=torch.float64, device=device), shift.reshape(1, n).contiguous(),
                                          torch.empty(es.factor_moment_count(p), dtype=torch.float64, device=device) if p else None, self.factor_names)
        self.spans = [o.shard_of(r) for r in range(o.world)]
        self.largest_shard = max(hi - lo for lo, hi in self.spans)
        self.send = torch.empty((self.largest_shard, n), dtype=torch.float64, device=device) if o.world > 1 else None
        self.recv = torch.empty((o.world, self.largest_shard * n), dtype=torch.float64, device=device) if o.world > 1 else None
        self.merged = self.result = None
        self.bytes_per_rank = 8 * self.largest_shard * n if o.world > 1 else 0

    def take(self, a: int, b: int, values, status) -> None:
        o = self.owner
        glo = o.geometry_range[0]
        if self.on_device:
            o.dp.curves_ensemble(values, steps_per_geometry=o.steps, status=status, out=self.local, first_row=a - glo)
            return
        part = es.curves_host(*self.host_tables(a, b, values, status), **self.host_kw)
        self.local.features[a - glo : b - glo] = torch.from_numpy(part.features)
        self.local.count[a - glo : b - glo] = torch.from_numpy(part.count)

    def exchange(self) -> None:
        """ONE all-gather of the feature rows (padded to the largest shard), then the reduction of the whole table on every rank."""
        o, acc = self.owner, self.acc
        table = self.local.table()
        if o.world > 1:
            self.send.fill_(float("nan"))
            self.send[: table.shape[0]] = table
            all_gather_flat(self.send.view(-1), o.group, out=self.recv)
            n = table.shape[1]
            table = torch.cat([self.recv[r, : (hi - lo) * n].reshape(hi - lo, n) for r, (lo, hi) in enumerate(self.spans)])
        self.result = None
        if self.on_device:
            o.dp.reduce_ensemble(table, steps_per_geometry=1, factors=self.factors, out=acc)
            self.merged = acc
            return
        self.merged = es.reduce_host(table.numpy()[:, None, :], None, None if self.factors is None else self.factors.numpy(), acc.shift.numpy(), 0,
                                     self.factor_names)

    def curve_stats(self):
        if self.merged is None:
            raise RuntimeError("no step() yet")
        if self.result is None:
            self.result = self.merged.finalize()
        return self.result


class Front(_Stage):
    """``front=dict(objectives=, source=, screened=)``: the nondominated front, chunk by chunk after the screen and the curves of the
    chunk; chunks merge into the rank's front.  At the end of a step the ranks all-gather their local front rows - id, M raw
    values and a member byte per slot, padded to the largest shard, and one more row with seen | candidates - and every rank runs
    the pass once more over the gathered rows: only comparisons, so the same bits on every rank."""

    def __init__(self, owner, front):
        super().__init__(owner)
        o = owner
        k = len(o.metric_index)
        self.source, self.screened = front.get("source", "table"), bool(front.get("screened", False))
        objectives = [tuple(ob) for ob in front["objectives"]]
        self.steps, self.columns = o.steps, k
        if self.source == "curves":
            # (column, field, sense ...) of the feature table [G, K * 12], one step per geometry
            self.steps, self.columns = 1, k * es.CURVE_FIELDS
            for ob in objectives:
                if len(ob) < 3 or any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) for x in ob[:2]) \
                        or not (0 <= ob[0] < k and 0 <= ob[1] < es.CURVE_FIELDS):
                    raise ValueError(f"front=: a curves objective is (column, field, sense ...) with column in [0, {k}) and field in "
                                     f"[0, {es.CURVE_FIELDS}), got {ob!r}")
            objectives = [(0, int(ob[0]) * es.CURVE_FIELDS + int(ob[1])) + ob[2:] for ob in objectives]
        self.objectives = objectives
        _, self.sense, self.target = es.check_front_arguments(objectives, self.steps, self.columns, o.n_geom)
        m = self.m = int(self.sense.size)
        # the gathered rows as a table of their own: one step, M columns, the senses and targets as given
        self.row_objectives = [(0, i, int(self.sense[i])) + ((float(self.target[i]),) if self.sense[i] == es.FRONT_TARGET else ()) for i in range(m)]
        self.largest_shard = max(hi - lo for lo, hi in (o.shard_of(r) for r in range(o.world)))
        self.local = self.merged = self.result = None
        self.bytes_per_rank = 8 * (self.largest_shard + 1) * (m + 2) if o.world > 1 else 0

    def take(self, a: int, b: int, values, status) -> None:
        o = self.owner
        rows = slice(a - o.geometry_range[0], b - o.geometry_range[0])
        if self.source == "curves":
            values, status = o.stages["curves"].local.table()[rows], None
        mask = None
        if self.screened:
            screen = o.stages["screen"]
            mask = (screen.run.flags if self.on_device else screen.part.flags)[rows]
        if self.on_device:
            part = o.dp.front_ensemble(values, steps_per_geometry=self.steps, objectives=self.objectives, status=status, mask=mask, geometry_offset=a)
        else:
            n = b - a
            part = es.front_host(values.reshape(n, self.steps, self.columns).cpu().numpy(), None if status is None else status.reshape(n, self.steps).cpu().numpy(),
                                 self.objectives, mask, None, a)
        self.local = self.local.merge(part) if self.taken else part

    def exchange(self) -> None:
        o, m, n, mine = self.owner, self.m, self.largest_shard, self.local
        self.result = None
        if o.world == 1:
            self.merged = mine
            return
        send = torch.zeros((n + 1, m + 2), dtype=torch.float64, device=o.device)
        if self.on_device:
            held = min(mine.capacity, n)
            send[:held, 0] = mine.front_index[:held].view(torch.float64)  # (the id's int64 bits)
            send[:held, 1 : m + 1] = mine.front_values[:held]
            send[:held, m + 1] = mine.member()[:held].to(torch.float64)
            send[n, :2] = mine.tally[:2].view(torch.float64)
        else:
            held = mine.index.size
            send[:held, 0] = torch.from_numpy(mine.index.astype(np.int64)).view(torch.float64)
            send[:held, 1 : m + 1] = torch.from_numpy(np.ascontiguousarray(mine.values))
            send[:held, m + 1] = 1.0
            send[n, :2] = torch.from_numpy(mine.tally[:2].astype(np.int64)).view(torch.float64)
        table = all_gather_flat(send.view(-1), o.group).view(o.world, n + 1, m + 2)
        rows = table[:, :n].reshape(o.world * n, m + 2)
        ids = rows[:, 0].contiguous().view(torch.int64)
        mask = (rows[:, m + 1] == 0).to(torch.uint8)
        counts = table[:, n, :2].contiguous().view(torch.int64).sum(dim=0)
        if self.on_device:
            merged = o.dp.front_ensemble(rows[:, 1 : m + 1], steps_per_geometry=1, objectives=self.row_objectives, mask=mask, index=ids)
            merged.tally[:2] = counts
            merged.dominated = None
        else:
            merged = es.front_host(rows[:, 1 : m + 1].numpy()[:, None, :], None, self.row_objectives, mask.numpy(), ids.numpy())
            merged.tally[:2] = counts.numpy()
            merged.dominated = None
        self.merged = merged

    def front(self):
        if self.merged is None:
            raise RuntimeError("no step() yet")
        if self.result is None:
            self.result = self.merged.finalize() if self.on_device else self.merged
        return self.result
