"""
Multi-GPU: the batch (sweep steps x geometries) shards by contiguous index range, one process
per GPU; there is no data-path collective while solving.  The single exchange step is an
all-gather of the solved positions (RCCL over xGMI on the GPU box; gloo in the CPU tests).
"""

from __future__ import annotations

from dataclasses import dataclass

import torch
import torch.distributed as dist


def shard_range(n_items: int, rank: int, world_size: int) -> tuple[int, int]:
    """Contiguous, balanced ``[lo, hi)`` block of ``n_items`` for ``rank`` (first ranks get the remainder)."""
    if not 0 <= rank < world_size:
        raise ValueError("rank out of range")
    base, extra = divmod(n_items, world_size)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def all_gather_rows(local: torch.Tensor, n_total: int, group=None, spans=None) -> torch.Tensor:
    """
    Gather per-rank row blocks into the full ``[n_total, ...]`` tensor on every rank.  The blocks are
    ``shard_range`` of the rows unless ``spans`` gives every rank's ``[lo, hi)`` explicitly (geometry-major
    shards: whole geometries per rank).  Uneven blocks are padded to the largest one for the collective.
    """
    if not dist.is_available() or not dist.is_initialized() or dist.get_world_size(group) == 1:
        if local.shape[0] != n_total:
            raise ValueError("single-process gather expects the full batch")
        return local
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    if spans is None:
        spans = [shard_range(n_total, r, world) for r in range(world)]
    if len(spans) != world or spans[0][0] != 0 or spans[-1][1] != n_total or \
            any(a[1] != b[0] for a, b in zip(spans, spans[1:])):
        raise ValueError("spans must tile [0, n_total) in rank order")
    lo, hi = spans[rank]
    if local.shape[0] != hi - lo:
        raise ValueError(f"rank {rank}: expected {hi - lo} rows, got {local.shape[0]}")
    biggest = max(b - a for a, b in spans)
    if hi - lo < biggest:
        pad = torch.zeros((biggest - (hi - lo), *local.shape[1:]), dtype=local.dtype, device=local.device)
        local = torch.cat([local, pad], dim=0)
    local = local.contiguous()
    gathered = torch.empty((world * biggest, *local.shape[1:]), dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(gathered, local, group=group)
    if n_total == world * biggest:
        return gathered
    return torch.cat([gathered[r * biggest : r * biggest + (b - a)] for r, (a, b) in enumerate(spans)], dim=0)


def _takes_host_tensors(tensor: torch.Tensor, group) -> bool:
    """A device tensor over gloo (ranks rehearsing on one GPU): the collective is given a host copy."""
    return tensor.is_cuda and dist.get_backend(group) == "gloo"


def broadcast_from_rank_zero(tensor: torch.Tensor, group=None) -> torch.Tensor:
    """Rank 0's ``tensor`` on every rank, on the device it was given on."""
    src = dist.get_global_rank(group, 0) if group is not None else 0
    sent = tensor.cpu() if _takes_host_tensors(tensor, group) else tensor
    dist.broadcast(sent, src, group=group)
    return sent.to(tensor.device)


def all_reduce_sum(tensor: torch.Tensor, group=None) -> None:
    """``tensor`` summed over the ranks, in place; a world of one does nothing."""
    if _world(group)[0] == 1:
        return
    if _takes_host_tensors(tensor, group):
        host = tensor.cpu()
        dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
        tensor.copy_(host)
    else:
        dist.all_reduce(tensor, op=dist.ReduceOp.SUM, group=group)


def all_gather_flat(local: torch.Tensor, group=None, out: torch.Tensor | None = None) -> torch.Tensor:
    """Every rank's flat ``local [words]`` as the rows of one ``[world, words]`` table (``out``, or a new one) on ``local``'s device."""
    if out is None:
        out = torch.empty((dist.get_world_size(group), local.numel()), dtype=local.dtype, device=local.device)
    if _takes_host_tensors(local, group):
        host = torch.empty(out.numel(), dtype=out.dtype)
        dist.all_gather_into_tensor(host, local.cpu(), group=group)
        out.view(-1).copy_(host)
    else:
        dist.all_gather_into_tensor(out.view(-1), local, group=group)
    return out


class GatherPipeline:
    """
    Overlaps the exchange step with the next solve: the all-gather of step ``k`` runs on the
    collective's own stream (RCCL over xGMI) while the solve kernel of step ``k + 1`` fills the
    other of two output slots.  In steady state a step costs ``max(solve, all-gather)`` instead of
    their sum.  Equal shards only (``n_total`` divisible by the world size).

        pipe = GatherPipeline(rows_per_rank, (n_out, 3), torch.float64, device)
        for k in range(steps):
            out = pipe.begin(k)        # local buffer of this step (waits for the gather that last read it)
            ... launch the solve into ``out`` on the current stream ...
            pipe.submit(k)             # asynchronous all-gather of ``out``
        full = pipe.drain()            # gathered positions of the last step, all exchanges complete
    """

    def __init__(self, rows_per_rank: int, tail_shape, dtype, device, group=None, depth: int = 2,
                 collective_at_world_one: bool = False):
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        # one rank with an initialised process group can still run the collective (a one-GPU box rehearsing the RCCL
        # path: communicator set-up, stream ordering of the pipeline, the expand on the gathered buffer)
        self.exchange = self.world > 1 or (collective_at_world_one and dist.is_available() and dist.is_initialized())
        self.depth = depth
        self.local = [torch.empty((rows_per_rank, *tail_shape), dtype=dtype, device=device) for _ in range(depth)]
        self.full = [torch.empty((rows_per_rank * self.world, *tail_shape), dtype=dtype, device=device)
                     if self.exchange else None for _ in range(depth)]
        self.work = [None] * depth
        self.last = -1

    def begin(self, k: int) -> torch.Tensor:
        slot = k % self.depth
        if self.work[slot] is not None:
            self.work[slot].wait()  # NCCL: the current stream waits; gloo: the host does
            self.work[slot] = None
        return self.local[slot]

    def submit(self, k: int) -> None:
        slot = k % self.depth
        self.last = slot
        if self.exchange:
            self.work[slot] = dist.all_gather_into_tensor(self.full[slot], self.local[slot], group=self.group,
                                                          async_op=True)

    def drain(self) -> torch.Tensor:
        for slot in range(self.depth):
            if self.work[slot] is not None:
                self.work[slot].wait()
                self.work[slot] = None
        if self.last < 0:
            raise RuntimeError("nothing was submitted")
        return self.full[self.last] if self.exchange else self.local[self.last]


class FreeGatherPipeline:
    """
    The pipelined exchange of the bench step with the compact payload: the solve writes the FREE coordinates of its
    problems (``3 n_free`` doubles each, ``okx_solve_opts.output = OKX_OUTPUT_FREE``) straight into the send buffer, the
    all-gather of step ``k`` runs on the collective's stream while step ``k + 1`` solves into the other slot, and one
    ``expand`` per step rebuilds every rank's output records from the gathered block (fixed points from the design
    state, derived points re-evaluated: bit-identical to what the solver would have written) - 144 B instead of 360 B
    per double-wishbone solve on the links, no packing pass, no second copy of the local records.

        pipe = FreeGatherPipeline(rows_per_rank, n_out, n_free, expand, dtype, device)
        launches = [plan(out=buf, output=pipe.output) for buf in pipe.solve_buffers]
        for k in range(steps):
            pipe.begin(k)                          # the slot's previous exchange is complete, its buffers are free
            launches[k % len(launches)]()          # solve into pipe.solve_buffers[k % depth]
            pipe.submit(k)                         # asynchronous all-gather of what was just solved
        positions = pipe.drain()                   # [rows_per_rank * world, n_out, 3] of the last step

    ``expand(free [R, n_free, 3], out [R, n_out, 3])`` fills ``out`` (``DeviceProgram.expand``).  With one rank and no
    collective the solve writes its records itself (``output == "records"``) and ``drain`` returns them.
    """

    def __init__(self, rows_per_rank: int, n_out: int, n_free: int, expand, dtype, device, group=None, depth: int = 2,
                 collective_at_world_one: bool = False):
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        # one rank with an initialised process group can still run the collective (a one-GPU box rehearsing the RCCL
        # path: communicator set-up, stream ordering of the pipeline, the expand on the gathered buffer)
        self.exchange = self.world > 1 or (collective_at_world_one and dist.is_available() and dist.is_initialized())
        self.depth = depth
        self.expand = expand
        self.output = "free" if self.exchange else "records"
        width = n_free if self.exchange else n_out
        self.solve_buffers = [torch.empty((rows_per_rank, width, 3), dtype=dtype, device=device) for _ in range(depth)]
        self.gathered = [torch.empty((rows_per_rank * self.world, n_free, 3), dtype=dtype, device=device)
                         if self.exchange else None for _ in range(depth)]
        self.full = [torch.empty((rows_per_rank * self.world, n_out, 3), dtype=dtype, device=device)
                     if self.exchange else None for _ in range(depth)]
        self.work = [None] * depth
        self.pending = [False] * depth  # gathered free coordinates not expanded yet
        self.last = -1
        self.bytes_sent_per_step = rows_per_rank * n_free * 3 * torch.empty((), dtype=dtype).element_size() if self.exchange else 0

    def _finish(self, slot: int) -> None:
        if self.work[slot] is not None:
            self.work[slot].wait()  # NCCL: the current stream waits; gloo: the host does
            self.work[slot] = None
        if self.pending[slot]:
            self.expand(self.gathered[slot], self.full[slot])
            self.pending[slot] = False

    def begin(self, k: int) -> torch.Tensor:
        slot = k % self.depth
        self._finish(slot)  # the previous exchange of this slot: the positions of that step are complete now
        return self.solve_buffers[slot]

    def submit(self, k: int) -> None:
        slot = k % self.depth
        self.last = slot
        if self.exchange:
            self.work[slot] = dist.all_gather_into_tensor(self.gathered[slot], self.solve_buffers[slot], group=self.group,
                                                          async_op=True)
            self.pending[slot] = True

    def drain(self) -> torch.Tensor:
        for slot in range(self.depth):
            self._finish(slot)
        if self.last < 0:
            raise RuntimeError("nothing was submitted")
        return self.full[self.last] if self.exchange else self.solve_buffers[self.last]


@dataclass
class EnsembleShard:
    """What ``solve_sharded(..., hardpoints=...)`` returns next to the gathered positions."""

    local: object                      # BatchResult of this rank's geometries (exchange="free" with N > 1: free coordinates, no records)
    geometry_range: tuple              # [lo, hi) of the geometries this rank solved
    free_full: torch.Tensor | None     # gathered free coordinates [G * S, n_free, 3] (exchange="free")
    info_full: torch.Tensor | None     # gathered okx_info records [G * S, 40] uint8 (None with info="status")
    exchange_bytes_per_rank: int       # payload this rank contributed to the all-gather(s)
    status_full: torch.Tensor | None = None  # info="status": one byte per solve [G * S], the low byte of okx_info.flags


@dataclass
class _LocalShard:
    """This rank's part of a pipelined ensemble, shaped like the ``BatchResult`` of a compact solve."""

    free: torch.Tensor
    info_raw: torch.Tensor
    positions: object = None


def _world(group):
    world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
    return world, (dist.get_rank(group) if world > 1 else 0)


def aligned_shard_range(n_items: int, rank: int, world_size: int, align: int = 1) -> tuple[int, int]:
    """``shard_range`` in units of ``align`` items: both ends are multiples of ``align`` (the last end is ``n_items``)."""
    if align <= 1:
        return shard_range(n_items, rank, world_size)
    lo, hi = shard_range(-(-n_items // align), rank, world_size)
    return min(lo * align, n_items), min(hi * align, n_items)


def chunk_pieces(n_geom: int, world: int, chunks: int, align: int = 1) -> list:
    """
    The piece table of a chunked ensemble exchange, the same on every rank: ``pieces[k][r] = (g_lo, g_hi)`` - the
    geometries rank ``r`` solves in chunk ``k`` (its ``shard_range`` block cut into ``chunks`` contiguous runs; runs may
    be empty when a rank has fewer geometries than chunks).  ``align``: shards and runs are cut in units of ``align``
    geometries - every boundary is a multiple of it (whole pick-freeze families); 1 is the plain table.
    """
    table = []
    for k in range(chunks):
        row = []
        for r in range(world):
            lo, hi = aligned_shard_range(n_geom, r, world, align)
            a, b = aligned_shard_range(hi - lo, k, chunks, align)
            row.append((lo + a, lo + b))
        table.append(row)
    return table


class PlanTable:
    """
    A ``SamplePlan`` where ``ShardedEnsemble`` takes a hardpoint table ``[G, P, 3]``: a slice of geometries is DRAWN when it is
    asked for - by ``DeviceProgram.sample_ensemble`` into HBM, or by ``ensemble_sample.sample_host`` for a program without it (the
    CPU tests' stand-in) - so a rank draws only the geometries it rebinds.  A ``FamilyPlan`` (the pick-freeze ensemble of
    ``sobol=True``) is drawn through ``sample_families`` / ``families_host`` in the same way.
    """

    def __init__(self, device_program, plan):
        from .ensemble_sample import FamilyPlan

        self.dp, self.plan = device_program, plan
        self.families = isinstance(plan, FamilyPlan)
        self.shape = (int(plan.n_total), plan.n_points, 3)
        self.on_device = hasattr(device_program, "sample_families" if self.families else "sample_ensemble")
        self.device = device_program.device if self.on_device else torch.device("cpu")

    def draw(self, lo: int, hi: int, latents: bool = False, flags: bool = False):
        """``(hardpoints [n, P, 3], latents [n, Z] or None)`` of geometries ``[lo, hi)``, tensors on ``device``; with ``flags`` a third
        item, the sampler's flag bytes ``[n]`` uint8."""
        if self.on_device:
            run = (self.dp.sample_families if self.families else self.dp.sample_ensemble)(self.plan, lo, hi, latents=latents)
            return (run.hardpoints, run.latents, run.flags) if flags else (run.hardpoints, run.latents)
        from .ensemble_sample import families_host, sample_host

        table, lat, _, byte = (families_host if self.families else sample_host)(self.plan, lo, hi)
        out = (torch.as_tensor(table), torch.as_tensor(lat) if latents else None)
        return (*out, torch.as_tensor(byte)) if flags else out

    def __getitem__(self, rows):
        if not isinstance(rows, slice) or rows.step not in (None, 1):
            raise TypeError("a plan's table is read in slices of geometries")
        lo, hi, _ = rows.indices(self.shape[0])
        return self.draw(lo, max(lo, hi))[0]


class ShardedEnsemble:
    """
    BASELINE config 5 on N GPUs as a PIPELINE (geometry-major contiguous shards, one exchange of the
    solved states).  Every rank cuts its shard into ``chunks`` runs of whole geometries and, chunk by chunk,

      * solves chunk k on the compute stream - the solve writes the free coordinates (``okx_solve_opts.output = free``, the
        exchange's payload) and the info records straight into THEIR FINAL PLACE in the gathered arrays: nothing is packed,
        staged or copied on the sending side;
      * exchanges chunk k with every peer in ONE grouped point-to-point call (``batch_isend_irecv``: on RCCL a single
        ncclGroup, every peer over its own xGMI link at once, coordinates and info records together; the receives land in
        their final place too) while chunk k + 1 solves;
      * optionally (``records=True``) rebuilds the output records of chunk k's pieces on a third stream while chunk k + 1
        travels and chunk k + 2 solves.

    A step therefore costs about ``max(solve, exchange, expand)`` of the whole batch plus one chunk of each, instead of
    their sum.  ``records=False`` returns the gathered free coordinates (what a consumer that evaluates metrics per rank,
    or writes per-rank result files, needs) and skips the expand altogether.  ``info="status"`` exchanges ONE status byte
    per solve (the low byte of ``okx_info.flags``: converged / residual exceeded / failed / ill-conditioned) instead of the
    40-byte record - 145 instead of 184 bytes per double-wishbone solve on the links; the full records of the rank's own
    shard stay in ``info_local``.  Chunked and unchunked runs give the same bits: a chunk is just a smaller launch of the
    same independent solves.

    ``metric_columns=[(metric, target), ...]`` turns the ensemble into an EVALUATED one (the program must have
    ``enable_evaluation`` done): every rank runs the evaluated solve on its shard - solve, tangents, metric catalog and
    derivative columns in one launch, no positions written (``okx_solve_evaluated_batch``) - and what travels is the
    chosen columns alone, 8 bytes each per state, beside the status byte: ``(metric, None)`` the value of a metric (name
    from ``metrics.METRIC_NAMES`` or column index of the evaluation row), ``(metric, t)`` its derivative along target
    ``t``.  ``step()`` then returns ``metric_full [G * S, K]``; the rank's own complete evaluation rows stay in
    ``eval_local [n_local, 1 + T, 24]``.  This is the form of the sharded ensemble that scales: a sensitivity study wants
    camber gain and bump steer of every perturbed geometry, not 144 bytes of coordinates per state on every rank.

    ``reduce=True`` (with ``metric_columns``) ends the ensemble in an ANSWER instead of a table: every chunk's columns are
    reduced on the device right after its evaluated solve (``okx_ensemble_reduce``: count, sums, extremes and which geometry
    produced them, cross sums with the factors) and merged into the rank's accumulator; nothing per state is exchanged - no
    ``metric_full``, no status bytes - and ``step()`` ends with ONE all-gather of the accumulators, merged on every rank in
    rank order (fixed order, extremes travel with their indices: every rank ends with the same bits).  ``step()`` returns
    the ``ensemble_stats.EnsembleAccumulator``; ``stats()`` finalizes it.  ``factors``: None (moments and extremes only),
    ``[G, P]`` per-geometry factors of the WHOLE ensemble, or ``"hardpoints"``: ``hardpoints - hardpoints.mean(0)``
    restricted to the coordinates of authored points that vary (``factor_names`` says which).  ``shift``: the common shift
    of the sums ``[S, K]``; None: the evaluation of global geometry 0 on the kernel the ensemble is pinned to (rank 0 solves
    its S states once, here, and broadcasts the table), undefined entries 0.  The unmasked factor moments of a rank's
    geometries never change: they are summed once, here, on the host in ascending geometry order - so ``factor_acc`` repeats
    bit for bit from step to step, rank to rank and chunking to chunking, but agrees with a direct
    ``reduce_ensemble(factor_moments=True)`` of the same table (summed per slab on the device) to rounding only.

    ``hardpoints`` may be an ``ensemble_sample.SamplePlan`` instead of a table: the ensemble is then the plan's ``n_total``
    geometries and every rank DRAWS the rows it rebinds (``okx_ensemble_sample``: geometry g's draw depends on the seed and g
    alone, so the rows carry the same bits on every rank and for every world size) - no table is built on the host, uploaded
    or sent.  ``factors="sampled"`` (with a plan) takes the plan's latents as the factors, named ``"latent<z>"`` or, for a plan
    without ``mixing``, by its coordinates; they come out of the same draw as the rank's rows and stay on the device (one host
    copy feeds the factor moments).  Two routes still hold ALL geometries on every rank, as they do with a table: with records
    and more than one rank every rank rebinds (so draws) the whole ensemble, and ``curves=`` with factors reduces every rank's
    feature rows against the factors of all geometries, which each rank then draws once more, whole, and copies to the host.
    Either way the run equals, bit for bit, the run over the materialised table (``sample_host(plan)``) with the materialised
    latents as ``factors``.

    ``quantiles=(p, ...)`` (with ``reduce=True``; ``limits`` optional, ``[S, K, 2]`` / ``[K, 2]`` / ``[2]`` = (lo, hi)) adds the
    band and the yield: after the last chunk of a step the rank runs the select rounds (``okx_ensemble_select_count`` /
    ``_descend``) over its ``metric_local``, and per round the ranks SUM their int64 histograms (one ``all_reduce``; over
    gloo on a GPU through host tensors) before each descends its own copy of the state - integer sums, so every rank ends
    with the same bits whatever the world size and chunking.  ``quantiles()`` returns ``ensemble_stats.EnsembleQuantiles``;
    the traffic is ``select_exchange_bytes_per_rank`` (``exchange_bytes_per_rank`` stays the accumulators').  A rank
    without a geometry contributes a zero histogram.

    ``screen=True`` (with ``reduce=True`` and ``limits``; ``quantiles`` not needed; ``screen_scale``: ``[S, K]`` / ``[K]`` / a
    scalar, None: 1) adds the JOINT verdict per geometry (``okx_ensemble_screen``): right after a chunk's reduction its rows
    of ``metric_local`` are screened into this rank's per-geometry tables, tally and blame accumulate and the survivors are
    appended.  ``step()`` then ends with one integer ``all_reduce`` of ``tally | blame`` and one all-gather of the flag bytes
    (1 B per geometry, padded to the largest shard).  ``screen()`` returns the ``ensemble_stats.EnsembleScreen`` of the WHOLE
    ensemble - ``tally``, ``blame``, ``flags [G]``, ``passed`` -, the same bits on every rank whatever the world size and
    chunking; ``screen_local()`` this rank's ``margin`` / ``entry`` / ``pass_index`` tensors, which stay where they are;
    ``screen_exchange_bytes_per_rank`` what the rank sends.

    ``covariance=True`` or ``covariance=entries`` (with ``reduce=True``; ``entries``: N distinct indices ``s K + k`` of the
    chosen columns' table, ``True``: all ``S K``, at most 2048) adds how the entries move TOGETHER
    (``okx_ensemble_covariance``): right after a chunk's reduction, with the reduction's shift, its rows of ``metric_local``
    are accumulated into this rank's Gram matrix, sums and counts over the COMPLETE geometries (every selected entry
    counts).  ``step()`` then ends with one all-gather of ``gram | sum | counts``, merged on every rank in rank order - the
    same bits on every rank; different world sizes and chunkings agree to rounding, as the accumulators of the reduction
    do.  ``covariance()`` returns the ``ensemble_stats.EnsembleCovariance`` (mean, covariance, std, correlation),
    ``covariance_accumulator`` holds the merged tables and ``covariance_local_used`` this rank's per-geometry used bytes.
    ``covariance_exchange_bytes_per_rank`` is ``8 (N^2 + N + 2)`` - 8 MB at N = 1024 however few geometries there are, which
    is why a SUBSET of entries (a few steps of a few columns) is the intended use at scale; no rank ever holds the table.

    ``curves=dict(abscissa=..., scale=..., origin=0.0, degree=2, window=None)`` (with ``reduce=True``) adds what lies ALONG the
    sweep (``okx_ensemble_curves``): right after a chunk's reduction, every geometry's rows of ``metric_local`` become a row of
    12 curve characteristics per chosen column - fitted value, gradient and curvature at ``origin``, departure from the fitted
    shape, extremes and where they occur - in this rank's feature table.  ``abscissa`` is an index into ``metric_columns`` (every
    geometry against its own ``wheel_travel``) or a shared ``[S]`` table.  ``step()`` then ends with ONE more all-gather, of the
    feature rows themselves (96 bytes per geometry and column, padded to the largest shard - ``S / 12`` times less than the
    columns they came from), and every rank reduces the same table ``[G, K * 12]`` (one step per geometry,
    ``okx_ensemble_reduce`` with the factors of all geometries): the answer carries the same bits on every rank and for every
    world size and chunking.  The common shift is the feature row of the reduction's own shift table, so nobody solves again.
    ``curve_stats()`` returns the ``ensemble_stats.EnsembleStats`` of the features over ALL geometries, every table
    ``[1, K * 12]`` - moments, extremes with their geometry index and, with ``factors``, the sensitivities of gradients and
    curvatures to the hardpoints; ``curves_local()`` this rank's ``EnsembleCurves``, which stay
    where they are; ``curves_exchange_bytes_per_rank`` what the rank sends.

    ``front=dict(objectives=..., source="table" | "curves", screened=False)`` (with ``reduce=True``) adds WHICH geometries are worth
    keeping (``okx_ensemble_front``): the nondominated (Pareto) front on up to 8 objectives.  ``source="table"`` takes objectives
    ``(step, column, sense)`` / ``(step, column, "target", value)`` over ``metric_columns``; ``source="curves"`` (needs ``curves=``)
    takes ``(column, field, sense...)`` over the curve features; ``screened=True`` (needs ``screen=True``) lets only the geometries
    that pass the screen be candidates - its flag bytes are the mask, as they lie in HBM.  The stage runs after the screen and
    the curves of a chunk; chunks merge into the rank's front (``front(A u B) = front(front(A) u front(B))``, the same kernel
    again); ``step()`` ends with one all-gather of the local front rows - id, M values and a member byte, padded to the largest
    shard - and every rank runs the pass once more over the gathered rows.  All comparisons: the same bits on every rank and
    for every world size and chunking.  ``front()`` returns the ensemble's ``ensemble_stats.EnsembleFront``, ``front_local()`` this
    rank's run, ``front_exchange_bytes_per_rank`` what the rank sends.  At most 65536 geometries.

    ``sobol=True`` (with ``reduce=True`` and an ``ensemble_sample.FamilyPlan`` where the hardpoints go) adds WHICH FACTOR GROUP
    explains the variance (``okx_ensemble_sobol``): the ensemble is the plan's pick-freeze families, ``M = D + 2`` geometries
    each, drawn by ``okx_ensemble_sample_families``; shards and chunks are cut in whole families (``chunk_pieces(..., align=M)``),
    and right after a chunk's reduction its rows of ``metric_local`` are accumulated with the reduction's shift and the chunk's
    sampler flags as the mask.  ``step()`` then ends with one all-gather of the accumulators, added on every rank in ascending
    rank order - the same bits on every rank; world sizes and chunkings agree to rounding, exactly when the sums are exact.
    ``sobol()`` returns the ``ensemble_stats.EnsembleSobol`` (first-order and total-order indices per group and entry),
    ``sobol_accumulator`` the merged tables, ``sobol_exchange_bytes_per_rank`` what the rank sends.

    ``bootstrap=R`` (with ``sobol=True``; ``bootstrap_seed`` None: the plan's seed) adds HOW FAR TO TRUST those indices
    (``okx_ensemble_sobol_bootstrap``): ``R`` Poisson-bootstrap replicates of the Sobol' accumulators, each chunk right after the
    Sobol' stage took it.  A family's weight in a replicate is a pure function of (seed, global family index, replicate) - the
    chunk's ``family_offset`` is ``a // family_size`` - so every rank and chunking forms the same replicates, and ``step()`` ends with
    one more all-gather, added in ascending rank order.  ``sobol_bootstrap(level=0.95)`` returns the
    ``ensemble_stats.EnsembleSobolBootstrap`` (the replicates' indices, their standard deviations and percentile intervals),
    ``sobol_bootstrap_accumulator`` the merged tables, ``sobol_bootstrap_exchange_bytes_per_rank`` what the rank sends.  Families are
    resampled as independent units; under ``LHS`` they are not quite, so the intervals are on the conservative side.

    ``effects=n_bins`` or ``effects=dict(bins=B, edges=table)`` (with ``reduce=True`` and ``factors``) adds HOW an entry depends on each
    single factor beyond a straight line (``okx_ensemble_bin`` / ``okx_ensemble_effects``): count, sum and sum of squares of every entry
    over ``B`` equal-probability bins of every factor - the given-data estimator, from the ordinary ensemble and without a further
    solve.  The edges ``[P, B - 1]`` carry the same bits on every rank: with ``factors="sampled"`` they are the plan's own inverse CDFs
    at ``k / B`` (``ensemble_stats.effects_edges``), otherwise the order statistics of the factors of all geometries.  A chunk's factor
    rows are binned once; right after the chunk's reduction its rows of ``metric_local`` are accumulated with the reduction's shift
    and, when the ensemble was sampled, the sampler's flags as the mask.  ``step()`` then ends with one all-gather of the
    accumulators, added on every rank in ascending rank order - the same bits on every rank; on the device a rank's chunks continue
    every cell's chain, so chunkings of one rank carry the same bits; world sizes agree to rounding.  ``effects()`` returns the
    ``ensemble_stats.EnsembleEffects`` (conditional mean and spread per bin, first-order index per factor and entry),
    ``effects_accumulator`` the merged tables, ``effects_exchange_bytes_per_rank`` what the rank sends (``24 P B S K``).

    ``whatif=scenarios`` (with ``reduce=True``, a ``SamplePlan`` and ``factors="sampled"``) adds WHAT THE SCATTER AND THE YIELD BECOME when
    tolerances change (``okx_ensemble_tilt_weights`` / ``okx_ensemble_reweigh``): ``scenarios`` is the list of specs
    ``ensemble_sample.tolerance_scenarios`` takes (or its table); every geometry gets the likelihood ratio of its latents under each
    scenario - a chunk's weights are computed once - and right after the chunk's reduction (and screen) its rows of ``metric_local`` are
    accumulated as weighted sums with the reduction's shift, the sampler's flags as the mask, ``limits=`` when given and, with
    ``screen=True``, the screen's flag bytes as the verdict.  No further draw and no further solve.  ``step()`` then ends with one
    all-gather of the accumulators, added on every rank in ascending rank order - the same bits on every rank; world sizes and
    chunkings agree to rounding, exactly when the sums are exact.  ``whatif()`` returns the ``ensemble_stats.EnsembleWhatIf``,
    ``whatif_accumulator`` the merged tables, ``whatif_exchange_bytes_per_rank`` what the rank sends (``8 N (10 S K + 7)``).  It is refused for a
    ``FamilyPlan``, whose pick-freeze members are no draw of the plan's law.

    ``surface=True`` or ``surface=dict(degree=, interactions=, entries=, factors=)`` (with ``reduce=True`` and ``factors``) adds a POLYNOMIAL
    RESPONSE SURFACE of the selected entries on the factors (``okx_ensemble_basis`` / ``okx_ensemble_surface``): which pairs of factors act
    together, a model that predicts an entry at a perturbed geometry without a solve, and first-order, pairwise and total variance shares
    from one fit on the ordinary ensemble.  The basis comes from the plan's laws for ``factors="sampled"`` (orthonormal Hermite / Legendre
    polynomials of the latents), otherwise from the factor table of all geometries (standardised monomials; no variance shares).  A chunk's
    basis rows are built once, and right after the chunk's reduction its rows of ``metric_local`` are accumulated into the normal equations
    with the reduction's shift and the sampler's flags as the mask.  Default entries: all ``S K`` when that is at most 2048, else ``entries=``
    is asked for.  ``step()`` then ends with one all-gather of the accumulators, added on every rank in ascending rank order - the same bits
    on every rank; world sizes and chunkings agree to rounding, exactly when the sums are exact.  ``surface()`` returns the
    ``ensemble_stats.EnsembleSurface``, ``surface_accumulator`` the merged tables, ``surface_exchange_bytes_per_rank`` what the rank sends
    (``8 (T^2 + T N + N + 2)``).  It is refused for a ``FamilyPlan``: the pick-freeze rows are not an independent sample.
    """

    def __init__(self, device_program, hardpoints, targets, steps_per_geometry: int, *, group=None, chunks: int | None = None,
                 records: bool = True, relative_targets: bool = True, info: str = "full", direct: bool | None = None,
                 metric_columns=None, reduce: bool = False, factors=None, shift=None, quantiles=None, limits=None, screen: bool = False, screen_scale=None,
                 covariance=None, curves=None, front=None, sobol: bool = False, bootstrap: int | None = None, bootstrap_seed: int | None = None,
                 effects=None, whatif=None, surface=None, **solve_kw):
        from .ensemble_sample import FamilyPlan, SamplePlan

        self.plan = hardpoints if isinstance(hardpoints, (SamplePlan, FamilyPlan)) else None
        if sobol and not isinstance(self.plan, FamilyPlan):
            raise ValueError("sobol=True decomposes a pick-freeze ensemble: pass an ensemble_sample.FamilyPlan where the hardpoints go")
        if sobol and not reduce:
            raise ValueError("sobol=True accumulates the reduced ensemble: it needs reduce=True")
        if (bootstrap is not None or bootstrap_seed is not None) and (not sobol or bootstrap is None):
            raise ValueError("bootstrap= resamples the families of the Sobol' accumulators: it needs sobol=True (and bootstrap_seed needs bootstrap=)")
        if bootstrap is not None:
            from .ensemble_stats import check_replicates

            bootstrap = check_replicates("bootstrap=", bootstrap)
        # sobol=True: shards and chunks are cut in whole families
        self.align = self.plan.family_size if sobol else 1
        if self.plan is not None:
            hardpoints = PlanTable(device_program, self.plan)  # rows are drawn where they are asked for
        elif isinstance(factors, str) and factors == "sampled":
            raise ValueError("factors='sampled' takes the latents of a SamplePlan: pass the plan where the hardpoints go")
        if (reduce or factors is not None or shift is not None) and (metric_columns is None or not reduce):
            raise ValueError("reduce=True reduces metric columns: it needs metric_columns (and factors / shift need reduce=True)")
        if (screen or screen_scale is not None) and (not screen or not reduce or limits is None):
            raise ValueError("screen=True screens the reduced ensemble: it needs reduce=True and limits (and screen_scale needs screen=True)")
        if whatif is not None and (not reduce or isinstance(self.plan, FamilyPlan) or not (isinstance(factors, str) and factors == "sampled")):
            raise ValueError("whatif= reweighs the ensemble of a SamplePlan by its latents: it needs reduce=True, factors='sampled' and no FamilyPlan "
                             "(a pick-freeze family is not a draw of the plan's law)")
        if (quantiles is not None or (limits is not None and not screen and whatif is None)) and (not reduce or quantiles is None):
            raise ValueError("quantiles / limits select over the reduced ensemble: they need reduce=True (and limits need quantiles)")
        if covariance is False:
            covariance = None
        if covariance is not None and not reduce:
            raise ValueError("covariance= accumulates the reduced ensemble: it needs reduce=True")
        if effects is False:
            effects = None
        if effects is not None and (not reduce or factors is None):
            raise ValueError("effects= bins the factors of the reduced ensemble: it needs reduce=True and factors")
        if surface is False:
            surface = None
        if surface is not None and (not reduce or factors is None or isinstance(self.plan, FamilyPlan)):
            raise ValueError("surface= regresses the reduced ensemble on its factors: it needs reduce=True, factors and no FamilyPlan "
                             "(the pick-freeze rows are not an independent sample)")
        if curves is not None and not reduce:
            raise ValueError("curves= fits the reduced ensemble's columns: it needs reduce=True")
        if front is not None:
            from .ensemble_stats import FRONT_MAX_GEOMETRIES

            front = dict(front)
            unknown = set(front) - {"objectives", "source", "screened"}
            if not reduce:
                raise ValueError("front= ranks the reduced ensemble's geometries: it needs reduce=True")
            if unknown or "objectives" not in front or front.get("source", "table") not in ("table", "curves"):
                raise ValueError(f"front= takes objectives and optionally source ('table' or 'curves') and screened (got {sorted(front)})")
            if front.get("source", "table") == "curves" and curves is None:
                raise ValueError("front=dict(source='curves') reads the curve features: it needs curves=")
            if front.get("screened", False) and not screen:
                raise ValueError("front=dict(screened=True) takes the screen's flag bytes as its mask: it needs screen=True")
            if int(hardpoints.shape[0]) > FRONT_MAX_GEOMETRIES:
                raise ValueError(f"front= takes at most {FRONT_MAX_GEOMETRIES} geometries, the ensemble has {int(hardpoints.shape[0])}")
        self.reduce = bool(reduce)
        if metric_columns is not None:
            records, info = False, "status"   # nothing of the positions travels or is written
        self.dp = device_program
        self.group = group
        self.world, self.rank = _world(group)
        self.steps = int(steps_per_geometry)
        self.records = bool(records)
        program = device_program.program
        self.n_geom = int(hardpoints.shape[0])
        self.n_total = self.n_geom * self.steps
        if self.n_geom % self.align:
            raise ValueError(f"sobol=True: {self.n_geom} geometries are no whole families of {self.align}")
        glo, ghi = self.shard_of(self.rank)
        self.geometry_range = (glo, ghi)
        if chunks is None:
            # Up to 8 chunks, but never a chunk below ONE FULL ROUND of the solve kernel over the chip (one 64-problem
            # wavefront on each of the 4 x CUs SIMDs: 65536 problems on an MI355X) - a smaller launch takes the same ~45 us
            # with most SIMDs idle, and the pipeline loses more on its solve stage than it hides of the exchange
            # (tools/c5_pipeline_model.py: a rank's 131072 problems at N = 8 solve in 0.09 ms as one launch or two halves, in
            # 0.40 ms as 8 eighths).  Without a GPU (the CPU tests' stand-in) a round is 4096.
            dev = hardpoints.device if self.plan is not None else torch.as_tensor(hardpoints).device
            one_round = torch.cuda.get_device_properties(dev).multi_processor_count * 256 if dev.type == "cuda" else 4096
            # (the evaluated ensemble sends 33 B instead of 145 B per state and computes 1.5 x as long: its exchange hides
            #  behind the solve with two chunks, more only lengthen the solve - tools/c5_pipeline_model.py)
            most = 2 if metric_columns is not None else 8
            # (from the SMALLEST shard, a rank-independent number: the piece tables and the grouped send / receive calls
            #  must have the same chunk count on every rank, and uneven shards differ by one geometry)
            least = min(hi - lo for lo, hi in (self.shard_of(r) for r in range(self.world)))
            chunks = max(1, min(most, (least * self.steps) // one_round, least // self.align)) if self.world > 1 else 1
        self.chunks = max(1, int(chunks))
        # Kernel family and chain length are chosen ONCE, for the whole ensemble as one launch on one GPU (auto selection
        # goes by the problem count: a 16384-problem chunk of a million-problem ensemble would otherwise run the quad kernel
        # where the ensemble runs the lane kernel - same answers to 1e-9, other bits): every chunk on every rank is forced
        # to that choice, so chunked, unchunked, one-GPU and N-GPU runs of an ensemble agree bit for bit.
        if hasattr(device_program, "plan_launch"):
            if hasattr(device_program, "wait_ready"):
                device_program.wait_ready()  # (a program still on its interpreter kernels would pin every chunk to them)
            kernel, chain_len = device_program.plan_launch(self.n_total, steps_per_geometry=self.steps, geometry_tables=True,
                                                           evaluated=metric_columns is not None, **solve_kw)
            solve_kw = {**solve_kw, "kernel": kernel, "chain_len": chain_len}
        self.solve_kw = solve_kw
        self.pieces = chunk_pieces(self.n_geom, self.world, self.chunks, self.align)
        # per-geometry emission: the expand on the receiving side needs every geometry's fixed points (a small table,
        # replicated as SURVEY.md section 8e allows); without records only this rank's slice is rebound
        everyone = self.records and self.world > 1
        self.sampled_latents = None  # factors="sampled": this rank's rows of the plan's latents, where they were drawn
        self.sampled_flags = None    # a plan: this rank's rows of the sampler's flag bytes
        if self.plan is not None:
            # ONE draw: the rows this rank rebinds and, when they are the factors, their latents beside them
            lo, hi = (0, self.n_geom) if everyone else (glo, ghi)
            table, drawn, byte = hardpoints.draw(lo, hi, latents=isinstance(factors, str) and factors == "sampled", flags=True)
            if drawn is not None:
                self.sampled_latents = drawn[glo - lo : ghi - lo]
            self.sampled_flags = byte[glo - lo : ghi - lo]
        else:
            table = hardpoints if everyone else hardpoints[glo:ghi]
        gpos, gparam = device_program.rebind(table)
        self.gpos_all = gpos if everyone else None
        self.my_pos = gpos[glo:ghi] if everyone else gpos
        self.my_param = gparam[glo:ghi] if everyone else gparam
        targets = torch.as_tensor(targets)
        if relative_targets:
            self.local_targets = device_program.ensemble_targets(self.my_pos, targets)
        else:
            self.local_targets = targets[glo * self.steps : ghi * self.steps]
        device = self.device = self.my_pos.device
        if info not in ("full", "status"):
            raise ValueError("info must be 'full' or 'status'")
        self.metric_index = None
        if metric_columns is not None:
            from .metrics import METRIC_NAMES

            # (columns per evaluation row: 24 for a corner, 64 for a composed axle - left block | right block | axle metrics | roles)
            self.eval_columns = int(getattr(device_program, "eval_columns", 0) or 24)
            flat = []
            for metric, target in metric_columns:
                col = METRIC_NAMES.index(metric) if isinstance(metric, str) else int(metric)
                row = 0 if target is None else 1 + int(target)
                if not (0 <= col < self.eval_columns and 0 <= row <= program.n_targets):
                    raise ValueError(f"no evaluation entry ({metric!r}, {target!r})")
                flat.append(row * self.eval_columns + col)
            if not flat:
                raise ValueError("metric_columns is empty")
            self.metric_index = torch.tensor(flat, dtype=torch.int64, device=device)

        self.status_only = info == "status" and (self.world > 1 or self.reduce)  # (one rank exchanges nothing: full records, a view of their flag byte)
        # ONE rank that wants records has nothing to exchange: its solves write the records themselves (`direct`; the gathered
        # free coordinates are then not kept - direct=False keeps the two-stage form, e.g. to compare the stages' bits)
        self.direct = (self.world == 1 and self.records and not self.status_only) if direct is None else bool(direct)
        if self.direct and (self.world > 1 or not self.records or self.status_only):
            raise ValueError("direct records need a world of one, records=True and info='full'")
        if self.metric_index is not None:
            if self.direct:
                raise ValueError("direct records and metric_columns exclude each other")
            n_local = (ghi - glo) * self.steps
            self.eval_local = torch.empty((n_local, 1 + program.n_targets, self.eval_columns), dtype=torch.float64, device=device)
            # (reduced: the chosen columns of the rank's own states only, the table the reduction reads)
            self.metric_full = None if self.reduce else torch.empty((self.n_total, len(self.metric_index)), dtype=torch.float64, device=device)
            self.metric_local = torch.empty((n_local, len(self.metric_index)), dtype=torch.float64, device=device) if self.reduce else None
        self.free_full = None if self.metric_index is not None else torch.empty((self.n_total, program.n_free, 3), dtype=torch.float64, device=device)
        # what travels beside the coordinates: the 40-byte info records, or one status byte per solve (then the records of
        # this rank's own shard are kept in `info_local`)
        self.info_full = None if self.status_only else torch.empty((self.n_total, 40), dtype=torch.uint8, device=device)
        self.status_full = torch.empty((self.n_total,), dtype=torch.uint8, device=device) if self.status_only and not self.reduce else None
        self.info_local = torch.empty(((ghi - glo) * self.steps, 40), dtype=torch.uint8, device=device) if self.status_only else None
        self.positions = torch.empty((self.n_total, program.n_out, 3), dtype=torch.float64, device=device) if self.records else None
        self.expand_stream = torch.cuda.Stream(device=device) if device.type == "cuda" and self.records and not self.direct else None
        if self.direct:
            self.free_full = None
        if info == "status" and not self.status_only:
            self.status_full, self.info_local = self.info_full[:, 32], self.info_full
        payload = program.n_free * 24 if self.metric_index is None else 8 * len(self.metric_index)
        self.exchange_bytes_per_rank = (ghi - glo) * self.steps * (payload + (1 if self.status_only else 40)) if self.world > 1 else 0
        # host time per chunk: the solve as a pre-bound launch (DeviceProgram.plan), the expands of a chunk's pieces (one per
        # rank) as ONE HIP graph replayed from the second step on
        self._plans = {}
        self._expand_graphs = {}
        self.use_graphs = device.type == "cuda"
        self.p2p_groups = self.p2p_ops = 0  # grouped point-to-point calls / operations issued so far
        # the stages of a reduced ensemble that are switched on, by name and in the order they run in (ensemble_stages.py)
        self.stages = {}
        self.select_probs = None
        self.screening, self.covarying = bool(screen), covariance is not None
        if self.reduce:
            from . import ensemble_stages as stages

            first = self.stages["reduce"] = stages.Reduction(self, hardpoints, targets, relative_targets, factors, shift)
            self.local_accumulator, self.exchange_bytes_per_rank = first.local, first.bytes_per_rank
            self.factor_names, self.n_factors, self.my_factors = first.factor_names, first.n_factors, first.my_factors
            if sobol:
                self.stages["sobol"] = stages.Sobol(self)
                if bootstrap is not None:
                    self.stages["sobol_bootstrap"] = stages.SobolBootstrap(self, bootstrap, self.plan.plan.seed if bootstrap_seed is None else bootstrap_seed)
            if quantiles is not None:
                stage = self.stages["select"] = stages.Selection(self, quantiles, limits)
                self.select_probs, self.select_limits = stage.probs, stage.limits
            if self.screening:
                stage = self.stages["screen"] = stages.Screening(self, limits, screen_scale)
                self.screen_limits, self.screen_scale = stage.limits, stage.scale
            if self.covarying:
                stage = self.stages["covariance"] = stages.Covariance(self, covariance)
                self.covariance_entries = stage.entries
            if effects is not None:
                self.stages["effects"] = stages.Effects(self, effects)
            if whatif is not None:
                self.stages["whatif"] = stages.WhatIf(self, whatif, limits)
            if surface is not None:
                self.stages["surface"] = stages.Surface(self, surface)
            if curves is not None:
                self.stages["curves"] = stages.Curves(self, dict(curves))
            if front is not None:
                self.stages["front"] = stages.Front(self, front)
        sent = {name: stage.bytes_per_rank for name, stage in self.stages.items()}
        self.select_exchange_bytes_per_rank, self.screen_exchange_bytes_per_rank = sent.get("select", 0), sent.get("screen", 0)
        self.covariance_exchange_bytes_per_rank = sent.get("covariance", 0)
        self.effects_exchange_bytes_per_rank = sent.get("effects", 0)
        self.whatif_exchange_bytes_per_rank = sent.get("whatif", 0)
        self.surface_exchange_bytes_per_rank = sent.get("surface", 0)
        self.curves_exchange_bytes_per_rank = sent.get("curves", 0)
        self.front_exchange_bytes_per_rank = sent.get("front", 0)
        self.sobol_exchange_bytes_per_rank = sent.get("sobol", 0)
        self.sobol_bootstrap_exchange_bytes_per_rank = sent.get("sobol_bootstrap", 0)

    # ---- reduce=True: the stages of ensemble_stages.py; what they hold and answer, by the names it has always had ----

    accumulator = property(lambda self: self.stages["reduce"].merged, doc="The merged accumulator of the last ``step()`` (``reduce=True``).")
    covariance_accumulator = property(lambda self: self.stages["covariance"].merged, doc="The merged covariance tables of the last ``step()``; None before.")

    def shard_of(self, rank: int) -> tuple:
        """``[lo, hi)`` of the geometries rank ``rank`` owns: ``shard_range``, cut in whole families with ``sobol=True``."""
        return aligned_shard_range(self.n_geom, rank, self.world, self.align)

    sobol_accumulator = property(lambda self: self.stages["sobol"].merged, doc="The merged Sobol' accumulator of the last ``step()`` (``sobol=True``); None before.")

    def sobol(self):
        """``ensemble_stats.EnsembleSobol`` of the WHOLE ensemble after the last ``step()`` (``sobol=True``): first-order and total-order
        indices of every factor group per (step, column) entry.  The same bits on every rank."""
        if "sobol" not in self.stages:
            raise ValueError("sobol() needs sobol=True")
        return self.stages["sobol"].sobol()

    sobol_bootstrap_accumulator = property(lambda self: self.stages["sobol_bootstrap"].merged,
                                           doc="The merged bootstrap replicates of the Sobol' accumulator of the last ``step()`` (``bootstrap=R``); None before.")

    def sobol_bootstrap(self, level: float = 0.95):
        """``ensemble_stats.EnsembleSobolBootstrap`` of the WHOLE ensemble after the last ``step()`` (``sobol=True, bootstrap=R``): the indices of
        every replicate, their standard deviations and the percentile intervals at ``level``.  The same bits on every rank."""
        if "sobol_bootstrap" not in self.stages:
            raise ValueError("sobol_bootstrap() needs sobol=True and bootstrap=R")
        return self.stages["sobol_bootstrap"].sobol_bootstrap(level)

    effects_accumulator = property(lambda self: self.stages["effects"].merged,
                                   doc="The merged main-effects accumulator of the last ``step()`` (``effects=``); None before.")

    def effects(self):
        """``ensemble_stats.EnsembleEffects`` of the WHOLE ensemble after the last ``step()`` (``effects=``): per factor, bin and entry the
        conditional mean and spread, per factor and entry the first-order index.  The same bits on every rank."""
        if "effects" not in self.stages:
            raise ValueError("effects() needs effects=n_bins")
        return self.stages["effects"].effects()

    whatif_accumulator = property(lambda self: self.stages["whatif"].merged,
                                  doc="The merged what-if accumulator of the last ``step()`` (``whatif=``); None before.")

    def whatif(self):
        """``ensemble_stats.EnsembleWhatIf`` of the WHOLE ensemble after the last ``step()`` (``whatif=``): per scenario and entry the reweighted
        mean, spread, effective sample size, standard error and yield; per scenario the joint yield and the mean weight.  The same bits on
        every rank."""
        if "whatif" not in self.stages:
            raise ValueError("whatif() needs whatif=scenarios")
        return self.stages["whatif"].whatif()

    surface_accumulator = property(lambda self: self.stages["surface"].merged,
                                   doc="The merged response-surface accumulator of the last ``step()`` (``surface=``); None before.")

    def surface(self):
        """``ensemble_stats.EnsembleSurface`` of the WHOLE ensemble after the last ``step()`` (``surface=``): per entry the coefficients of the
        basis terms, R^2 and the residual spread; with an orthonormal basis the first-order, pairwise and total variance shares.  The same
        bits on every rank."""
        if "surface" not in self.stages:
            raise ValueError("surface() needs surface=True or surface=dict(...)")
        return self.stages["surface"].surface()

    def quantiles(self):
        """``ensemble_stats.EnsembleQuantiles`` of the last ``step()`` (``quantiles=...``): the same bits on every rank."""
        if self.select_probs is None:
            raise ValueError("quantiles() needs quantiles=(p, ...)")
        return self.stages["select"].quantiles()

    def screen(self):
        """``ensemble_stats.EnsembleScreen`` of the WHOLE ensemble after the last ``step()`` (``screen=True``): ``tally``, ``blame``,
        ``flags [G]`` and ``passed``; ``margin`` / ``entry`` stay with their ranks (``screen_local``).  The same bits on every rank."""
        if not self.screening:
            raise ValueError("screen() needs screen=True")
        return self.stages["screen"].screen()

    def screen_local(self) -> dict:
        """This rank's tables of the last ``step()``: ``flags`` / ``margin`` / ``entry [n_local]``, ``pass_index`` (ascending global
        indices of its geometries that pass, ``pass_count`` of them) - tensors where the table lives, nothing is copied."""
        if not self.screening:
            raise ValueError("screen_local() needs screen=True")
        return self.stages["screen"].screen_local()

    @property
    def covariance_local_used(self) -> torch.Tensor:
        """This rank's used byte per geometry of the last ``step()`` (``covariance=``), where the table lives."""
        if not self.covarying:
            raise ValueError("covariance_local_used needs covariance=")
        return self.stages["covariance"].local.used

    def covariance(self):
        """``ensemble_stats.EnsembleCovariance`` of the WHOLE ensemble after the last ``step()`` (``covariance=``): count, mean,
        covariance, std and correlation of the selected entries over the complete geometries.  The same bits on every rank."""
        if not self.covarying:
            raise ValueError("covariance() needs covariance=True or covariance=entries")
        return self.stages["covariance"].covariance()

    def curves_local(self):
        """This rank's ``ensemble_stats.EnsembleCurves`` of the last ``step()`` (``curves=``): ``features [n_local, K, 12]`` and ``count
        [n_local, K]``, tensors where the table lives; ``.table()`` feeds the other ensemble passes with ``steps_per_geometry=1``."""
        if "curves" not in self.stages:
            raise ValueError("curves_local() needs curves=")
        return self.stages["curves"].local

    def curve_stats(self):
        """``ensemble_stats.EnsembleStats`` of the curve features over the WHOLE ensemble after the last ``step()`` (``curves=``), every
        table ``[1, K * 12]``: entry ``k * 12 + f`` is field f of column k.  The same bits on every rank."""
        if "curves" not in self.stages:
            raise ValueError("curve_stats() needs curves=")
        return self.stages["curves"].curve_stats()

    def front_local(self):
        """This rank's front run of the last ``step()`` (``front=``), its chunks merged: ``ensemble_device.EnsembleFronting`` of device
        tensors, or ``ensemble_stats.EnsembleFront`` on a CPU ensemble; nothing is copied."""
        if "front" not in self.stages:
            raise ValueError("front_local() needs front=")
        return self.stages["front"].local

    def front(self):
        """``ensemble_stats.EnsembleFront`` of the WHOLE ensemble after the last ``step()`` (``front=``): the ids and raw objective
        values of the geometries no other geometry beats, ``tally`` = seen, candidates, members.  The same bits on every rank."""
        if "front" not in self.stages:
            raise ValueError("front() needs front=")
        return self.stages["front"].front()

    def stats(self):
        """``ensemble_stats.EnsembleStats`` of the last ``step()`` (``reduce=True``): the merged accumulator, finalized on the host."""
        if not self.reduce:
            raise ValueError("stats() needs reduce=True")
        return self.accumulator.finalize()

    def _rows(self, span):
        return slice(span[0] * self.steps, span[1] * self.steps)

    def _solve_chunk(self, k: int) -> None:
        glo = self.geometry_range[0]
        a, b = self.pieces[k][self.rank]
        if b <= a:
            return
        rows = self._rows((a, b))
        local = slice((a - glo) * self.steps, (b - glo) * self.steps)
        if self.metric_index is not None:
            self._solve_chunk_evaluated(k, a, b, rows, local)
            return
        out = self.positions[rows] if self.direct else self.free_full[rows]
        info = self.info_local[local] if self.status_only else self.info_full[rows]
        shape = "records" if self.direct else "free"
        if out.is_cuda and hasattr(self.dp, "plan"):
            stream = torch.cuda.current_stream(out.device).cuda_stream
            bound = self._plans.get(k)
            if bound is None or bound[0] != stream:  # (a plan launches on the stream that was current when it was made)
                bound = (stream, self.dp.plan(self.local_targets[local], geom_pos=self.my_pos[a - glo : b - glo],
                                              geom_row_param=self.my_param[a - glo : b - glo], steps_per_geometry=self.steps,
                                              output=shape, out=out, info_out=info, **self.solve_kw))
                self._plans[k] = bound
            bound[1]()
            if self.status_only:
                self.status_full[rows] = info[:, 32]
            return
        res = self.dp.solve(self.local_targets[local], geom_pos=self.my_pos[a - glo : b - glo], geom_row_param=self.my_param[a - glo : b - glo],
                            steps_per_geometry=self.steps, output=shape, out=out, info_out=info, **self.solve_kw)
        # (a stand-in program of the CPU tests returns fresh tensors instead of filling the buffers it was given)
        got = res.positions if self.direct else res.free
        if got.data_ptr() != out.data_ptr():
            out.copy_(got)
        if res.info_raw.data_ptr() != info.data_ptr():
            info.copy_(res.info_raw)
        if self.status_only:
            self.status_full[rows] = info[:, 32]  # (okx_info.flags is the int32 at byte 32: its low byte carries every flag)

    def _solve_chunk_evaluated(self, k: int, a: int, b: int, rows, local) -> None:
        """The evaluated solve of one chunk (no positions written) and its chosen columns into their place in the gathered table."""
        glo = self.geometry_range[0]
        info = self.info_local[local] if self.status_only else self.info_full[rows]
        ev = self.eval_local[local]
        kw = dict(geom_pos=self.my_pos[a - glo : b - glo], geom_row_param=self.my_param[a - glo : b - glo], steps_per_geometry=self.steps,
                  output="none", info_out=info, eval_out=ev, **self.solve_kw)
        if ev.is_cuda and hasattr(self.dp, "plan_evaluated"):
            stream = torch.cuda.current_stream(ev.device).cuda_stream
            bound = self._plans.get(k)
            if bound is None or bound[0] != stream:
                bound = (stream, self.dp.plan_evaluated(self.local_targets[local], **kw))
                self._plans[k] = bound
            bound[1]()
        else:
            res = self.dp.solve_evaluated(self.local_targets[local], **kw)
            if res.eval.data_ptr() != ev.data_ptr():  # (the CPU tests' stand-in returns fresh tensors)
                ev.copy_(res.eval)
            if res.info_raw.data_ptr() != info.data_ptr():
                info.copy_(res.info_raw)
        if self.reduce:
            torch.index_select(ev.view(ev.shape[0], -1), 1, self.metric_index, out=self.metric_local[local])
            for stage in self.stages.values():
                stage.rows(a, b, local)
            return
        torch.index_select(ev.view(ev.shape[0], -1), 1, self.metric_index, out=self.metric_full[rows])
        if self.status_only:
            self.status_full[rows] = info[:, 32]

    def _exchange_chunk(self, k: int) -> list:
        if self.world == 1 or self.reduce:  # (reduced: nothing per state travels; the accumulators go once, at the end of the step)
            return []
        if self.device.type == "cuda" and dist.get_backend(self.group) == "gloo":
            return self._exchange_chunk_through_the_host(k)
        ops = []
        mine = self.pieces[k][self.rank]
        for peer in range(self.world):
            if peer == self.rank:
                continue
            dst = dist.get_global_rank(self.group, peer) if self.group is not None else peer
            theirs = self.pieces[k][peer]
            beside = self.status_full if self.status_only else self.info_full
            payload = self.free_full if self.metric_index is None else self.metric_full
            if mine[1] > mine[0]:
                ops.append(dist.P2POp(dist.isend, payload[self._rows(mine)], dst, self.group))
                ops.append(dist.P2POp(dist.isend, beside[self._rows(mine)], dst, self.group))
            if theirs[1] > theirs[0]:
                ops.append(dist.P2POp(dist.irecv, payload[self._rows(theirs)], dst, self.group))
                ops.append(dist.P2POp(dist.irecv, beside[self._rows(theirs)], dst, self.group))
        if ops:  # (what a bench line / a test reports: grouped calls issued and operations inside them, since construction)
            self.p2p_groups += 1
            self.p2p_ops += len(ops)
        return dist.batch_isend_irecv(ops) if ops else []

    def _exchange_chunk_through_the_host(self, k: int) -> list:
        """Device tensors over gloo (two ranks rehearsing on one GPU: gloo's point-to-point calls take host tensors): the
        same pieces, staged through host copies, complete on return."""
        mine = self.pieces[k][self.rank]
        ops, landing = [], []
        for peer in range(self.world):
            if peer == self.rank:
                continue
            dst = dist.get_global_rank(self.group, peer) if self.group is not None else peer
            theirs = self.pieces[k][peer]
            for full in (self.free_full if self.metric_index is None else self.metric_full, self.status_full if self.status_only else self.info_full):
                if mine[1] > mine[0]:
                    ops.append(dist.P2POp(dist.isend, full[self._rows(mine)].cpu(), dst, self.group))
                if theirs[1] > theirs[0]:
                    host = torch.empty_like(full[self._rows(theirs)], device="cpu")
                    ops.append(dist.P2POp(dist.irecv, host, dst, self.group))
                    landing.append((full[self._rows(theirs)], host))
        if ops:
            self.p2p_groups += 1
            self.p2p_ops += len(ops)
        for w in (dist.batch_isend_irecv(ops) if ops else []):
            w.wait()
        for device_rows, host in landing:
            device_rows.copy_(host)
        return []

    def _expand_chunk(self, k: int, works: list) -> None:
        def run():
            for w in works:
                w.wait()  # NCCL: this stream waits for the transfers; gloo: the host does
            pieces()

        def pieces():
            for r in range(self.world):
                a, b = self.pieces[k][r]
                if b <= a:
                    continue
                rows = self._rows((a, b))
                gp = self.gpos_all[a:b] if self.gpos_all is not None else self.my_pos[a - self.geometry_range[0] : b - self.geometry_range[0]]
                got = self.dp.expand(self.free_full[rows], out=self.positions[rows], geom_pos=gp, steps_per_geometry=self.steps)
                if got.data_ptr() != self.positions[rows].data_ptr():
                    self.positions[rows].copy_(got)

        if self.expand_stream is None:
            run()
            return
        self.expand_stream.wait_stream(torch.cuda.current_stream(self.expand_stream.device))  # (the own piece was solved there)
        with torch.cuda.stream(self.expand_stream):
            graph = self._expand_graphs.get(k)
            if not self.use_graphs or self.world == 1:
                run()
            elif graph is None:
                run()  # the first step: plain launches (nothing lazy inside a capture), the second step captures
                self._expand_graphs[k] = "warm"
            else:
                for w in works:
                    w.wait()
                if graph == "warm":
                    try:
                        graph = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(graph, stream=self.expand_stream, capture_error_mode="thread_local"):
                            pieces()  # (a linear graph: forking the pieces onto side streams inside the capture made the
                            #  replay SLOWER on this runtime - 0.39 against 0.31 ms for 16 nodes, EXPERIMENTS.md section 2)
                    except Exception:  # capture refused: stay with plain launches
                        self.use_graphs = False
                        torch.cuda.synchronize(self.expand_stream.device)
                        pieces()
                        return
                    self._expand_graphs[k] = graph
                graph.replay()

    def diagnose(self, roles, *, capacity: int = 4096, residual_tolerance: float = 1e-3):
        """
        The sweep diagnostics (``DeviceProgram.diagnose``, ``okx_diagnose_sweeps_batch``) of THIS RANK's shard after a
        ``step()``, where its records lie - the free coordinates the solve wrote (or the records of a direct one-rank
        ensemble), the shard's info records, every geometry's own design table - and an all-gather of the 80-byte summaries
        (sweeps never straddle ranks: the partition is by whole geometries).  Returns ``(summary_full [G, 80] uint8,
        issues, count)``: the summaries of every geometry on every rank; the issue records and their count stay this
        rank's own, their ``sweep`` field counted from ``geometry_range[0]``.  Not for an evaluated ensemble
        (``metric_columns``): it writes no positions.
        """
        if self.metric_index is not None:
            raise ValueError("an evaluated ensemble (metric_columns) keeps no positions to diagnose")
        glo, ghi = self.geometry_range
        rows = self._rows((glo, ghi))
        positions, layout = (self.positions[rows], "records") if self.direct else (self.free_full[rows], "free")
        info = self.info_local if self.status_only else self.info_full[rows]
        if ghi > glo:
            summary, issues, count = self.dp.diagnose(positions, info, steps_per_sweep=self.steps, layout=layout, geom_pos=self.my_pos,
                                                      roles=roles, capacity=capacity, residual_tolerance=residual_tolerance)
        else:
            summary = torch.empty((0, 80), dtype=torch.uint8, device=self.device)
            issues = torch.empty((0, 40), dtype=torch.uint8, device=self.device)
            count = torch.zeros(1, dtype=torch.int64, device=self.device)
        if self.world > 1:
            spans = [shard_range(self.n_geom, r, self.world) for r in range(self.world)]
            summary = all_gather_rows(summary, self.n_geom, self.group, spans=spans)
        return summary, issues, count

    def exchange_only(self):
        """The exchange stage alone (every chunk's grouped point-to-point call on whatever the buffers hold, waited for): what
        a step costs beyond its compute when nothing overlaps - a bench figure, not part of a step."""
        pending = []
        for k in range(self.chunks):
            pending += self._exchange_chunk(k)
        for w in pending:
            w.wait()

    def step(self):
        """One pass over the whole ensemble: returns ``positions`` (``records=True``) or the gathered free coordinates."""
        pending = []
        for stage in self.stages.values():
            stage.begin_step()
        for k in range(self.chunks):
            self._solve_chunk(k)
            works = self._exchange_chunk(k)
            if self.records and not self.direct:
                self._expand_chunk(k, works)
            else:
                pending += works
        for w in pending:
            w.wait()
        if self.expand_stream is not None:
            torch.cuda.current_stream(self.expand_stream.device).wait_stream(self.expand_stream)
        if self.reduce:
            # every rank, with or without a geometry, in this order: the accumulators' all-gather, the Sobol' accumulators' all-gather, the select rounds' all-reduces,
            # the screen's all-reduce and all-gather, the covariance's all-gather, the effects' all-gather, the curve features' all-gather, the front
            # rows' all-gather
            for stage in self.stages.values():
                stage.end_step()
            return self.accumulator
        if self.metric_index is not None:
            return self.metric_full
        return self.positions if self.records else self.free_full


def solve_sharded(device_program, targets_full: torch.Tensor, gather=True, group=None, *, hardpoints=None,
                  steps_per_geometry: int = 0, exchange: str = "free", relative_targets: bool | None = None,
                  chunks: int | None = None, info: str = "full", **solve_kw):
    """
    Solve this rank's index block and (optionally) all-gather the solved positions.

    Without ``hardpoints``: ``targets_full [B, T]`` absolute targets of one geometry, sharded by contiguous index
    range; returns ``(positions, local_result)``.

    With ``hardpoints [G, P, 3]`` (BASELINE config 5: perturbed geometries x sweep steps): the
    batch is **geometry-major**, a rank owns whole geometries ``shard_range(G, rank, world)``.  The rank rebinds
    its slice of the hardpoint table on the device (per-geometry problem emission, reference
    ``suspensions/corner/double_wishbone.py:259-308``), builds its targets, solves, and the exchange step gathers
    ``exchange="free"`` the free coordinates (``3 n_free`` doubles per solve; every rank then rebuilds all positions
    with ``expand`` from the replicated, rebound hardpoint table) or ``"positions"`` the output records
    themselves, plus the 40-byte info records.  ``targets_full`` is either ``[S, T]`` RELATIVE displacements
    applied to every geometry's own design coordinates (the reference's relative target mode) or ``[G * S, T]``
    absolute values (``relative_targets`` says which; ``None`` infers it from the row count, absolute when both
    fit); ``steps_per_geometry`` = S.  Returns ``(positions [G * S, n_out, 3], EnsembleShard)``.
    The compact exchange runs as a pipeline (``ShardedEnsemble``): the shard is cut into ``chunks`` runs of whole
    geometries (default: up to 8), chunk k + 1 solves while chunk k travels - coordinates and info records in one grouped
    point-to-point call, straight from and into their final place - and chunk k - 1 is expanded on a third stream.
    ``gather="free"`` skips the expand and returns the gathered free coordinates ``[G * S, n_free, 3]`` instead of the
    records (``EnsembleShard.free_full`` holds them either way); ``info="status"`` exchanges one status byte per solve
    instead of the 40-byte record (``EnsembleShard.status_full``; ``local.info_raw`` keeps this rank's full records).
    Uneven geometry counts need no padding.
    """
    world, rank = _world(group)
    if hardpoints is None:
        n_total = targets_full.shape[0]
        lo, hi = shard_range(n_total, rank, world)
        result = device_program.solve(targets_full[lo:hi], **solve_kw)
        positions = all_gather_rows(result.positions, n_total, group) if gather else result.positions
        return positions, result
    if exchange not in ("free", "positions"):
        raise ValueError("exchange must be 'free' or 'positions'")
    if gather == "free" and exchange != "free":
        raise ValueError("gather='free' returns the compact exchange's payload: exchange must be 'free'")
    steps = int(steps_per_geometry)
    n_geom = int(hardpoints.shape[0])
    if steps <= 0:
        raise ValueError("an ensemble needs steps_per_geometry > 0")
    program = device_program.program
    glo, ghi = shard_range(n_geom, rank, world)
    targets_full = torch.as_tensor(targets_full)
    relative = relative_targets if relative_targets is not None else \
        (targets_full.shape[0] == steps and n_geom * steps != steps)
    if targets_full.shape[0] != (steps if relative else n_geom * steps):
        raise ValueError("targets must be [S, T] relative displacements or [G * S, T] absolute values")
    if gather and world > 1 and exchange == "free":
        pipe = ShardedEnsemble(device_program, hardpoints, targets_full, steps, group=group, chunks=chunks,
                               records=gather != "free", relative_targets=relative, info=info, **solve_kw)
        result = pipe.step()
        own = pipe._rows(pipe.geometry_range)
        local = _LocalShard(pipe.free_full[own], pipe.info_local if pipe.status_only else pipe.info_full[own])
        return result, EnsembleShard(local, pipe.geometry_range, pipe.free_full, pipe.info_full, pipe.exchange_bytes_per_rank,
                                     pipe.status_full)
    # Per-geometry emission.  The expand on the receiving side needs every geometry's fixed points, so with the
    # compact exchange the (small: G x P x 24 B) hardpoint table is rebound in full on every rank — replicated
    # inputs, as SURVEY.md section 8e allows; otherwise only this rank's slice.
    everyone = gather and world > 1 and exchange == "free"
    table = hardpoints if everyone else hardpoints[glo:ghi]
    gpos, gparam = device_program.rebind(table)
    my_pos = gpos[glo:ghi] if everyone else gpos
    my_param = gparam[glo:ghi] if everyone else gparam
    if relative:
        local_targets = device_program.ensemble_targets(my_pos, targets_full)
    else:
        local_targets = targets_full[glo * steps : ghi * steps]
    # compact exchange: the solve writes the free coordinates alone (okx_solve_opts.output = OKX_OUTPUT_FREE) - they ARE the
    # payload, and one expand of the gathered block rebuilds every rank's records, this rank's own included
    compact = gather and world > 1 and exchange == "free"
    result = device_program.solve(local_targets, geom_pos=my_pos, geom_row_param=my_param, steps_per_geometry=steps,
                                  **(dict(solve_kw, output="free") if compact else solve_kw))
    if not gather or world == 1:
        return result.positions, EnsembleShard(result, (glo, ghi), None, result.info_raw if gather else None, 0)
    n_total = n_geom * steps
    spans = [tuple(steps * g for g in shard_range(n_geom, r, world)) for r in range(world)]
    info_full = all_gather_rows(result.info_raw, n_total, group, spans)
    sent = result.info_raw.numel() * result.info_raw.element_size()
    if not compact:
        positions = all_gather_rows(result.positions, n_total, group, spans)
        sent += result.positions.numel() * result.positions.element_size()
        return positions, EnsembleShard(result, (glo, ghi), None, info_full, sent)
    sent += result.free.numel() * result.free.element_size()
    free_full = all_gather_rows(result.free, n_total, group, spans)
    positions = device_program.expand(free_full, geom_pos=gpos, steps_per_geometry=steps)
    return positions, EnsembleShard(result, (glo, ghi), free_full, info_full, sent)
