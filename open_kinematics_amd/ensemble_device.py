"""
The device passes over an evaluated ensemble, host side.  ``EnsembleReductions`` is the mixin ``batch.DeviceProgram`` takes them
from; the host forms of what they return are described in ``ensemble_stats.py``.  Tensors stay in HBM; nothing here copies a
table to the host.

=============================  ====================  ==============================================
pass (``okx_ensemble_...``)    prepare call          result
=============================  ====================  ==============================================
``sample_ensemble``            -                     ``EnsembleSample`` (of a ``SamplePlan``)
``sample_families``            -                     ``EnsembleSample`` (of a ``FamilyPlan``)
``reduce_ensemble``            -                     ``ensemble_stats.EnsembleAccumulator``
``select_ensemble``            ``select_prepare``    ``EnsembleSelection``
``screen_ensemble``            ``screen_prepare``    ``EnsembleScreening``
``covariance_ensemble``        -                     ``ensemble_stats.CovarianceAccumulator``
``curves_ensemble``            ``curves_prepare``    ``ensemble_stats.EnsembleCurves``
``front_ensemble``             ``front_prepare``     ``EnsembleFronting``
``sobol_ensemble``             -                     ``ensemble_stats.SobolAccumulator``
``bootstrap_weights``          -                     ``uint8 [n_rows, R]`` tensor
``sobol_bootstrap_ensemble``   -                     ``ensemble_stats.SobolBootstrapAccumulator``
``effects_ensemble``           ``bin_factors``       ``ensemble_stats.EffectsAccumulator``
``tilt_weights``               ``tilt_prepare``      ``float64 [G, N]`` tensor
``reweigh_ensemble``           ``tilt_weights``      ``ensemble_stats.ReweighAccumulator``
``surface_ensemble``           ``basis_factors``     ``ensemble_stats.SurfaceAccumulator``
``predict_ensemble``           ``upload_surface``    ``(out [G, N], valid [G])`` tensors
``validate_surface``           ``upload_surface``    ``ensemble_stats.SurfaceValidation``
=============================  ====================  ==============================================

Every pass takes ``out=``, the result of an earlier call or of its prepare call; the tables it holds are checked in one place
(``EnsembleReductions._check_tables``) before anything is launched.
"""

from __future__ import annotations

import ctypes as C
import weakref
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .ensemble_stats import (CURVE_FIELDS, EFFECTS_FIELDS, ENS_FIELDS, FRONT_TARGET, PREDICT_RESIDUAL, PREDICT_VALUE, REWEIGH_FIELDS, REWEIGH_JOINT_FIELDS, REWEIGH_MAX_SCENARIOS,
                             SELECT_MAX_PROBS, SOBOL_FIELDS, SOBOL_MAX_GROUPS, CovarianceAccumulator, EffectsAccumulator, EnsembleAccumulator, EnsembleCurves,
                             ReweighAccumulator, SobolAccumulator, SobolBootstrapAccumulator, SurfaceAccumulator, SurfaceBasis, SurfaceValidation, _host_f64, broadcast_limits,
                             broadcast_scale, check_covariance_arguments, check_effects_arguments, check_front_arguments, check_replicates, check_reweigh_limits,
                             check_predict_arguments, check_surface_arguments, check_surface_basis, factor_moment_count, validation_from_terms)

F64, I64, I32, U8 = torch.float64, torch.int64, torch.int32, torch.uint8


@dataclass
class EnsembleSelection:
    """
    What ``DeviceProgram.select_ensemble`` returns and its round-level calls work on, device tensors: ``probs [Q]`` and
    ``limits [S, K, 2]`` (or None) as uploaded, ``order [S, K, Q, 2]`` the order statistics below / above every quantile,
    ``count [S, K]`` and ``outside [S, K, 2]`` (or None) int64; ``state`` / ``hist`` (``select_prepare(rounds=True)``) the
    opaque state and the int64 histogram ``[S, K, 2 Q, bins]`` of ``okx_ensemble_select_count``.
    """

    probs_host: np.ndarray
    probs: torch.Tensor
    limits: torch.Tensor | None
    order: torch.Tensor
    count: torch.Tensor
    outside: torch.Tensor | None
    state: torch.Tensor | None = None
    hist: torch.Tensor | None = None

    @property
    def shape(self) -> tuple:
        """``(S, K, Q)``."""
        return tuple(self.order.shape[:3])

    def finalize(self):
        """Host copy, interpolated: ``ensemble_stats.EnsembleQuantiles``."""
        from .ensemble_stats import quantiles_from_order

        return quantiles_from_order(self.probs_host, self.order.cpu().numpy(), self.count.cpu().numpy(),
                                    None if self.outside is None else self.outside.cpu().numpy())


@dataclass
class EnsembleScreening:
    """
    What ``DeviceProgram.screen_ensemble`` returns, device tensors: ``limits [S, K, 2]`` and ``scale [S, K]`` (or None) as
    uploaded; per geometry ``flags [G]`` uint8, ``margin [G]`` float64 and ``entry [G]`` int32; per ensemble ``tally [4]`` and
    ``blame [S, K, 2]`` int64, ``pass_index [capacity]`` int64 (the ascending global indices of the geometries that pass;
    slots beyond ``min(pass_count, capacity)`` are never written) and ``pass_count [1]`` int64, the survivors found.
    """

    limits: torch.Tensor
    scale: torch.Tensor | None
    flags: torch.Tensor
    margin: torch.Tensor
    entry: torch.Tensor
    tally: torch.Tensor
    blame: torch.Tensor
    pass_index: torch.Tensor
    pass_count: torch.Tensor

    @property
    def shape(self) -> tuple:
        """``(S, K)``."""
        return tuple(self.blame.shape[:2])

    def finalize(self):
        """Host copy: ``ensemble_stats.EnsembleScreen`` (``passed`` holds the survivors that fit the capacity)."""
        from .ensemble_stats import EnsembleScreen

        tally = self.tally.cpu().numpy()
        n = min(int(self.pass_count.item()), self.pass_index.shape[0])
        seen = min(int(tally[0]), self.flags.shape[0])  # (accumulated chunks fill the tables from the front)
        return EnsembleScreen(self.flags[:seen].cpu().numpy(), self.margin[:seen].cpu().numpy(), self.entry[:seen].cpu().numpy(), tally,
                              self.blame.cpu().numpy(), self.pass_index[:n].cpu().numpy())


@dataclass
class EnsembleFronting:
    """
    What ``DeviceProgram.front_ensemble`` returns, device tensors: per geometry ``dominated [G]`` int32 (None for a merged
    run); per ensemble ``tally [3]`` int64 (seen, candidates, front members), ``front_index [capacity]`` int64 and
    ``front_values [capacity, M]`` float64 - the ids and the raw table values of the front members in ascending row order;
    slots beyond ``min(tally[2], capacity)`` are never written.  ``entries`` / ``sense`` / ``target`` are the HOST arrays the launch
    reads; ``overflow [1]`` bool says that a run this one was merged from did not fit its capacity.
    """

    owner: object
    entries: np.ndarray
    sense: np.ndarray
    target: np.ndarray
    dominated: torch.Tensor | None
    tally: torch.Tensor
    front_index: torch.Tensor
    front_values: torch.Tensor
    overflow: torch.Tensor | None = None

    @property
    def capacity(self) -> int:
        return int(self.front_index.shape[0])

    def member(self) -> torch.Tensor:
        """``[capacity]`` bool, on the device: the slot holds a front member."""
        return torch.arange(self.capacity, device=self.tally.device) < self.tally[2]

    def truncated(self) -> torch.Tensor:
        """``[1]`` bool, on the device: the front (or one it was merged from) did not fit its capacity."""
        over = self.tally[2:3] > self.capacity
        return over if self.overflow is None else over | self.overflow

    def merge(self, other: "EnsembleFronting") -> "EnsembleFronting":
        """The front of the union of the two runs' front rows, by the SAME kernel over their ``front_values`` (one step, M
        columns, the senses and targets as given), the ids through ``d_index`` and the unused slots masked by a byte table
        built on the device from the counts - no host read.  ``seen`` and ``candidates`` add; no per-geometry ``dominated``."""
        if not (np.array_equal(self.sense, other.sense) and np.array_equal(self.target, other.target)):
            raise ValueError("fronts of different objectives")
        rows = torch.cat([self.front_values, other.front_values])
        ids = torch.cat([self.front_index, other.front_index])
        mask = (~torch.cat([self.member(), other.member()])).to(torch.uint8)
        objectives = [(0, i, int(s)) + ((float(t),) if s == FRONT_TARGET else ()) for i, (s, t) in enumerate(zip(self.sense, self.target))]
        out = self.owner.front_ensemble(rows, steps_per_geometry=1, mask=mask, index=ids, objectives=objectives)
        out.tally[:2] = self.tally[:2] + other.tally[:2]
        out.dominated = None
        out.overflow = self.truncated() | other.truncated()
        return out

    def finalize(self):
        """Host copy, the only host read: ``ensemble_stats.EnsembleFront``.  Raises when the front did not fit the capacity."""
        from .ensemble_stats import EnsembleFront

        tally = self.tally.cpu().numpy()
        n = int(tally[2])
        if n > self.capacity or (self.overflow is not None and bool(self.overflow.item())):
            raise RuntimeError(f"the front was truncated: {n} members, capacity {self.capacity}")
        return EnsembleFront(None if self.dominated is None else self.dominated.cpu().numpy(), tally, self.front_index[:n].cpu().numpy(),
                             self.front_values[:n].cpu().numpy(), self.sense.copy(), self.target.copy())


class SampleGuard(C.Structure):
    """``okx_sample_guard``."""

    _fields_ = [("kind", C.c_int32), ("a", C.c_int32), ("b", C.c_int32), ("c", C.c_int32), ("eps", C.c_double), ("sign", C.c_double)]


@dataclass
class EnsembleSample:
    """
    What ``DeviceProgram.sample_ensemble`` returns, device tensors of the geometries ``[lo, hi)`` of a plan's ensemble:
    ``hardpoints [n, P, 3]`` (what ``rebind`` and ``ShardedEnsemble`` take), ``latents [n, Z]`` and ``delta [n, F]`` (None unless
    asked for; ``latents`` feed ``reduce_ensemble(factors=...)``) and ``flags [n]`` uint8 (None when an ``out=`` without them was passed; bit 0: no attempt satisfied the guards -
    a ``mask`` for ``front_ensemble``; bits 4-7: the attempt kept).
    """

    hardpoints: torch.Tensor
    latents: torch.Tensor | None
    delta: torch.Tensor | None
    flags: torch.Tensor | None
    lo: int = 0


@dataclass
class EffectBins:
    """
    What ``DeviceProgram.bin_factors`` returns and ``effects_ensemble`` takes, device tensors of ``G`` geometries and ``F`` factors:
    ``bins [G, F]`` uint8 (the bin of the geometry for the factor, 255: the factor is NaN), ``order [F, G]`` int32 (per factor the
    binned geometries bin by bin, ascending inside a bin; -1 behind them), ``offsets [F, n_bins + 1]`` int64 (where every bin starts)
    and ``edges [F, n_bins - 1]`` float64 as uploaded.
    """

    bins: torch.Tensor
    order: torch.Tensor
    offsets: torch.Tensor
    edges: torch.Tensor
    n_bins: int


@dataclass
class SurfaceBasisTable:
    """What ``basis_factors`` returns, device tensors: ``phi [G, T]`` float64 with unit column stride (rows may be strided: a view of a wider
    table), the basis rows of the geometries; ``valid [G]`` uint8, 0 where a factor of the geometry is not finite (its row of ``phi`` is then 0);
    ``law [P, 3]`` and ``terms [T, 4]``, the uploaded tables of ``basis`` (``ensemble_stats.SurfaceBasis``, host)."""

    phi: torch.Tensor
    valid: torch.Tensor
    law: torch.Tensor
    terms: torch.Tensor
    basis: SurfaceBasis


@dataclass
class SurfaceModel:
    """What ``upload_surface`` returns and ``predict_ensemble`` / ``validate_surface`` take, device tensors of a fitted surface of ``T`` terms,
    ``P`` factors and ``N`` entries: ``law [P, 3]``, ``terms [T, 4]`` int32, ``coefficients [T, N]``, ``shift [N]``, ``entries [N]`` int32 and
    ``whitener [T, T]`` (None when the fit carries none); ``basis`` and ``entries_host`` are the host forms the checks read."""

    law: torch.Tensor
    terms: torch.Tensor
    coefficients: torch.Tensor
    shift: torch.Tensor
    entries: torch.Tensor
    whitener: torch.Tensor | None
    basis: SurfaceBasis
    entries_host: np.ndarray


def _ptr(t: torch.Tensor | None, row: int = 0) -> C.c_void_p:
    """The address of ``t`` (None: 0); with ``row``, of that row of a contiguous table - what ``t[row:]`` starts at, without making the view."""
    if t is None:
        return C.c_void_p(0)
    return C.c_void_p(t.data_ptr() + row * t.stride(0) * t.element_size() if row else t.data_ptr())


def _rows(t) -> int:
    """The row count of a table that sets its own; of anything without rows -1, a size no tensor has."""
    return t.shape[0] if isinstance(t, torch.Tensor) and t.dim() else -1


def _as_f64(t, device) -> torch.Tensor:
    """A contiguous float64 tensor ON the device: always a snapshot of host data (synchronous copy), whatever its kind."""
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(np.asarray(t, dtype=np.float64))
    return t.to(device=device, dtype=torch.float64).contiguous()


class EnsembleReductions:
    """
    The ensemble passes of a ``DeviceProgram`` (a mixin).  They read column tables, not the constraint program: all they
    need of the object is ``self.lib`` (the loaded library) and ``self.device``.
    """

    def _ensemble_table(self, values, status, steps_per_geometry: int):
        """``(G, S, K, ld, status stride)`` of a column table view of an ensemble pass: ``values [G * S, K]`` float64 with
        unit column stride (rows may be strided), ``status [G * S]`` uint8 (may be strided) or None."""
        s = int(steps_per_geometry)
        if values.dim() != 2 or values.dtype != torch.float64 or values.device != self.device or (values.shape[1] > 1 and values.stride(1) != 1):
            raise ValueError("values must be a float64 [G * S, K] device tensor with unit column stride")
        b, k = values.shape
        if s < 1 or b % s:
            raise ValueError("bad steps_per_geometry")
        ld = values.stride(0) if b > 1 else max(k, values.stride(0))
        if ld < k:
            raise ValueError("rows of values overlap")
        stride = 0
        if status is not None:
            if status.dtype != torch.uint8 or status.dim() != 1 or status.shape[0] != b or status.device != self.device:
                raise ValueError("status must be a uint8 [G * S] device tensor")
            stride = status.stride(0) if b > 1 else 1
        return b // s, s, k, ld, stride

    def _ensemble_shift(self, shift, values, g: int, s: int, k: int) -> torch.Tensor:
        """The common shift ``[S, K]`` on the device; None: geometry 0 of the table, undefined entries 0 (no geometry: zeros)."""
        if shift is None:
            shift = torch.nan_to_num(values[:s], nan=0.0, posinf=0.0, neginf=0.0) if g else torch.zeros((s, k), dtype=torch.float64, device=self.device)
        return _as_f64(shift, self.device).reshape(s, k).contiguous()

    def _ensemble_scratch(self, which: str, need: int) -> torch.Tensor:
        """The scratch buffer of pass ``which`` (one per pass), at least ``need`` bytes."""
        if not hasattr(self, "_ensemble_buffers"):
            self._ensemble_buffers = {}
        held = self._ensemble_buffers.setdefault(which, [])
        if not held or held[-1].numel() < need:  # grow-only; a captured graph keeps the buffer it was captured with alive
            held.append(torch.empty(max(need, 8), dtype=torch.uint8, device=self.device))
        return held[-1]

    def _ensemble_call(self, name: str, *args) -> None:
        """``name(*args, stream)`` of the library on torch's current stream of the device, its status checked."""
        stream = torch.cuda.current_stream(self.device).cuda_stream
        with torch.cuda.device(self.device):
            rc = getattr(self.lib, name)(*args, C.c_void_p(stream))
        _lib.check(rc, name)

    def _check_tables(self, message: str, tables, optional=()) -> None:
        """The ``out=`` contract, checked HERE for every pass: each ``(tensor, shape or None, dtype)`` of ``tables`` is a
        contiguous torch tensor of that dtype (and shape) on ``self.device``; those of ``optional`` may also be None.  Metadata
        only - no allocation, no device work -, so a checked call stays legal inside a stream capture."""
        dev = self.device
        for specs, needed in ((tables, True), (optional, False)):
            for t, shape, dtype in specs:
                if t is None and not needed:
                    continue
                if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == dev and t.is_contiguous() and (shape is None or t.shape == shape)):
                    raise ValueError(message)

    def _check_mask(self, mask, g: int, contiguous: bool) -> int:
        """The stride of ``mask`` (None: 0), a uint8 ``[G]`` device tensor: contiguous, or strided with a positive stride."""
        if mask is None:
            return 0
        if mask.dtype != U8 or mask.dim() != 1 or mask.shape[0] != g or mask.device != self.device or (contiguous and not mask.is_contiguous()):
            raise ValueError("mask must be a contiguous uint8 [G] device tensor" if contiguous else "mask must be a uint8 [G] device tensor")
        stride = mask.stride(0) if g > 1 else 1
        if stride < 1:
            raise ValueError("mask must have a positive stride")
        return stride

    @staticmethod
    def _new_result(out, carried: tuple, what: str, accumulate: bool = False,
                    needs: str = "accumulate=True needs the accumulator to merge into (out=)") -> bool:
        """The "new or given" rule of every pass.  True: there is no ``out=`` and the result is to be made - then
        ``accumulate=True`` is refused; False: ``out=`` is given - then the arguments it ``carried`` itself must be None."""
        if out is None:
            if accumulate:
                raise ValueError(needs)
            return True
        for x in carried:
            if x is not None:
                raise ValueError(f"out= carries its own {what}")
        return False

    def reduce_ensemble(self, values, *, steps_per_geometry: int, status=None, factors=None, shift=None, geometry_offset: int = 0,
                        out=None, accumulate: bool = False, factor_moments: bool = True):
        """
        ``okx_ensemble_reduce``: the statistics accumulator (``ensemble_stats.EnsembleAccumulator``, device tensors) of a
        column table in HBM over its geometries.  ``values [G * S, K]`` float64 with unit column stride - the gathered
        ``metric_full`` of an evaluated ensemble, or a strided view of its evaluation rows (``eval[:, 0, :]``: nothing is
        copied, the row stride is passed on); ``status [G * S]`` uint8, the low byte of ``okx_info.flags`` (``info_raw[:, 32]``
        is fine), or None: every state accepted; ``factors [G, P]`` per-geometry factors or None; ``shift [S, K]`` the common
        shift of the sums (None: the table's own geometry 0, undefined entries 0 - partial accumulators that are merged
        later need ONE shift, pass it); ``geometry_offset`` the global index of the table's geometry 0.  ``out``: an
        accumulator to write (``accumulate=False``) or merge into (``True``); with it and a table shape seen before, the call
        allocates nothing and is legal inside a stream capture.  ``factor_moments=False`` skips the factor moments (a caller
        that merges chunks of fixed factors takes them once).
        """
        g, s, k, ld, stride = self._ensemble_table(values, status, steps_per_geometry)
        p = 0
        if factors is not None:
            factors = _as_f64(factors, self.device)
            if factors.dim() != 2 or factors.shape[0] != g:
                raise ValueError("factors must be [G, P]")
            factors = factors.contiguous()
            p = factors.shape[1]
        if self._new_result(out, (shift,), "shift", accumulate):
            out = EnsembleAccumulator(torch.empty((s, k, ENS_FIELDS + p), dtype=F64, device=self.device), self._ensemble_shift(shift, values, g, s, k),
                                      torch.empty(factor_moment_count(p), dtype=F64, device=self.device) if p and factor_moments else None)
        factor_acc = out.factor_acc if factor_moments and p else None
        self._check_tables(f"out must hold contiguous device tables [S, K, {ENS_FIELDS + p}] and [S, K]",
                           [(out.acc, (s, k, ENS_FIELDS + p), F64), (out.shift, (s, k), F64)], [(factor_acc, (factor_moment_count(p),), F64)])
        scratch = self._ensemble_scratch("reduce", int(self.lib.okx_ensemble_scratch_bytes(g, s, k, p)))
        self._ensemble_call("okx_ensemble_reduce", g, s, k, _ptr(values), ld, _ptr(status), stride, _ptr(factors), p, _ptr(out.shift),
                            int(geometry_offset), 1 if accumulate else 0, _ptr(out.acc), _ptr(factor_acc), _ptr(scratch), scratch.numel())
        return out

    # ---- okx_ensemble_select: exact order statistics and spec-limit counts (ensemble_stats.EnsembleQuantiles) ----

    def select_prepare(self, steps: int, n_columns: int, probs, limits=None, *, rounds: bool = False) -> "EnsembleSelection":
        """
        The tables of a select over ``[steps, n_columns]`` entries: ``probs`` (``[Q]`` in [0, 1]) and ``limits`` (``[S, K, 2]``,
        ``[K, 2]`` or ``[2]`` = (lo, hi), -inf / +inf leaves a side open; None: no limit counts) are validated by
        ``okx_ensemble_select_check`` on the host and uploaded ONCE; outputs are allocated.  ``rounds=True`` adds the state and
        the histogram the round-level calls (``select_begin`` / ``select_count`` / ``select_descend`` / ``select_finish``) work on.
        """
        s, k = int(steps), int(n_columns)
        p = np.ascontiguousarray(np.atleast_1d(_host_f64(probs)).reshape(-1))
        lim = None if limits is None else broadcast_limits(limits, s, k)
        rc = self.lib.okx_ensemble_select_check(p.ctypes.data_as(C.c_void_p), min(p.size, SELECT_MAX_PROBS + 1),
                                                None if lim is None else lim.ctypes.data_as(C.c_void_p), 0 if lim is None else s * k)
        _lib.check(rc, "okx_ensemble_select")
        q, dev = p.size, self.device
        run = EnsembleSelection(p, torch.as_tensor(p, device=dev), None if lim is None else torch.as_tensor(lim, device=dev),
                                torch.empty((s, k, q, 2), dtype=torch.float64, device=dev), torch.empty((s, k), dtype=torch.int64, device=dev),
                                None if lim is None else torch.empty((s, k, 2), dtype=torch.int64, device=dev))
        if rounds:
            run.state = torch.empty(max(1, int(self.lib.okx_ensemble_select_state_bytes(s, k, q))), dtype=torch.uint8, device=dev)
            run.hist = torch.empty((s, k, 2 * q, int(self.lib.okx_ensemble_select_hist_len(s, k, q)) // max(1, s * k * 2 * q)),
                                   dtype=torch.int64, device=dev)
        return run

    @property
    def select_rounds(self) -> int:
        return int(self.lib.okx_ensemble_select_rounds())

    def _select_tables(self, run: "EnsembleSelection", rounds: bool) -> tuple:
        """``(S, K, Q)`` of ``run``, its tables checked: those of ``select_ensemble``, and with ``rounds`` the state and the
        histogram the round-level calls work on."""
        message = "out must hold contiguous device tables probs [Q], limits [S, K, 2], order [S, K, Q, 2], count [S, K] and outside [S, K, 2]" \
            + (", state and hist [S, K, 2 Q, bins]" if rounds else "")
        order = run.order
        if not isinstance(order, torch.Tensor) or order.dim() != 4 or (run.outside is None) != (run.limits is None):
            raise ValueError(message)
        s, k, q = order.shape[:3]
        tables = [(run.probs, (q,), F64), (order, (s, k, q, 2), F64), (run.count, (s, k), I64)]
        if rounds:
            bins = int(self.lib.okx_ensemble_select_hist_len(s, k, q)) // max(1, s * k * 2 * q)
            tables += [(run.state, None, U8), (run.hist, (s, k, 2 * q, bins), I64)]
        self._check_tables(message, tables, [(run.limits, (s, k, 2), F64), (run.outside, (s, k, 2), I64)])
        if rounds and run.state.numel() < int(self.lib.okx_ensemble_select_state_bytes(s, k, q)):
            raise ValueError(message)
        return s, k, q

    def select_begin(self, run: "EnsembleSelection") -> None:
        """State and histogram of ``run`` zeroed on the stream (``okx_ensemble_select_begin``)."""
        s, k, q = self._select_tables(run, True)
        self._ensemble_call("okx_ensemble_select_begin", s, k, q, _ptr(run.state), _ptr(run.hist))

    def select_count(self, run: "EnsembleSelection", rnd: int, values, *, steps_per_geometry: int, status=None) -> None:
        """Round ``rnd`` over one chunk of geometries ``values [G' * S, K]``, added into ``run.hist`` (``okx_ensemble_select_count``)."""
        g, s, k, ld, stride = self._ensemble_table(values, status, steps_per_geometry)
        if (s, k) != run.shape[:2]:
            raise ValueError(f"the select was prepared for [S, K] = {list(run.shape[:2])}")
        self._select_tables(run, True)
        self._ensemble_call("okx_ensemble_select_count", int(rnd), g, s, k, _ptr(values), ld, _ptr(status), stride, run.shape[2],
                            _ptr(run.limits), _ptr(run.state), _ptr(run.hist))

    def select_descend(self, run: "EnsembleSelection", rnd: int) -> None:
        """``run.hist`` consumed and re-zeroed, the state advanced by one round (``okx_ensemble_select_descend``)."""
        s, k, q = self._select_tables(run, True)
        self._ensemble_call("okx_ensemble_select_descend", int(rnd), s, k, _ptr(run.probs), q, _ptr(run.state), _ptr(run.hist))

    def select_finish(self, run: "EnsembleSelection") -> "EnsembleSelection":
        """``run.order`` / ``count`` / ``outside`` written from the state (``okx_ensemble_select_finish``)."""
        s, k, q = self._select_tables(run, True)
        self._ensemble_call("okx_ensemble_select_finish", s, k, q, _ptr(run.state), _ptr(run.order), _ptr(run.count), _ptr(run.outside))
        return run

    def select_ensemble(self, values, *, steps_per_geometry: int, probs=None, status=None, limits=None, out=None):
        """
        ``okx_ensemble_select``: per (step, column) entry of a column table in HBM, over the geometries whose state counts
        (the rule of ``reduce_ensemble``), the two order statistics around every probability of ``probs`` - exact bits of
        table values - the count, and with ``limits`` the counts of values strictly below ``lo`` / above ``hi``.  ``values``
        and ``status`` as ``reduce_ensemble`` takes them (unit column stride; strided rows and a strided status byte are
        passed on, nothing is copied).  Returns an ``EnsembleSelection`` of device tensors (``order [S, K, Q, 2]``, ``count
        [S, K]``, ``outside [S, K, 2]`` or None); ``.finalize()`` copies it to the host and interpolates
        (``ensemble_stats.EnsembleQuantiles``).  ``out``: the selection of an earlier call or of ``select_prepare`` - it carries
        its own probabilities and limits; with it and a table shape seen before, the call uploads and allocates nothing and
        is legal inside a stream capture.  Bit-identical from run to run: integer counting only.
        """
        g, s, k, ld, stride = self._ensemble_table(values, status, steps_per_geometry)
        if self._new_result(out, (probs, limits), "probabilities and limits"):
            if probs is None:
                raise ValueError("probs is needed (or out=, which carries its own)")
            out = self.select_prepare(s, k, probs, limits)
        if out.shape[:2] != (s, k) or out.order.device != self.device:
            raise ValueError(f"out was prepared for [S, K] = {list(out.shape[:2])} on {out.order.device}")
        q = self._select_tables(out, False)[2]
        scratch = self._ensemble_scratch("select", int(self.lib.okx_ensemble_select_scratch_bytes(s, k, q)))
        self._ensemble_call("okx_ensemble_select", g, s, k, _ptr(values), ld, _ptr(status), stride, _ptr(out.probs), q, _ptr(out.limits),
                            _ptr(out.order), _ptr(out.count), _ptr(out.outside), _ptr(scratch), scratch.numel())
        return out

    # ---- okx_ensemble_screen: the joint spec-limit verdict of every geometry (ensemble_stats.EnsembleScreen) ----

    def screen_prepare(self, steps: int, n_columns: int, limits, scale=None, n_geometries: int = 0, capacity: int | None = None) -> "EnsembleScreening":
        """
        The tables of a screen over ``[steps, n_columns]`` entries and ``n_geometries`` geometries: ``limits`` (``[S, K, 2]``,
        ``[K, 2]`` or ``[2]`` = (lo, hi), -inf / +inf leaves a side open) and ``scale`` (``[S, K]``, ``[K]`` or a scalar, finite
        and > 0; None: 1) are validated by ``okx_ensemble_screen_check`` on the host and uploaded ONCE; the outputs are
        allocated, the survivor list with ``capacity`` slots (None: one per geometry).
        """
        s, k, g = int(steps), int(n_columns), int(n_geometries)
        if limits is None:
            raise ValueError("limits are needed: [S, K, 2], [K, 2] or [2] (lo, hi)")
        lim = broadcast_limits(limits, s, k)
        sc = None if scale is None else broadcast_scale(scale, s, k)
        rc = self.lib.okx_ensemble_screen_check(lim.ctypes.data_as(C.c_void_p), None if sc is None else sc.ctypes.data_as(C.c_void_p), s * k)
        _lib.check(rc, "okx_ensemble_screen")
        if g < 0 or (capacity is not None and int(capacity) < 0):
            raise ValueError("negative geometry count or capacity")
        dev = self.device
        cap = g if capacity is None else int(capacity)
        return EnsembleScreening(torch.as_tensor(lim, device=dev), None if sc is None else torch.as_tensor(sc, device=dev),
                                 torch.empty(g, dtype=torch.uint8, device=dev), torch.empty(g, dtype=torch.float64, device=dev),
                                 torch.empty(g, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int64, device=dev),
                                 torch.zeros((s, k, 2), dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int64, device=dev),
                                 torch.zeros(1, dtype=torch.int64, device=dev))

    def screen_ensemble(self, values, *, steps_per_geometry: int, limits=None, status=None, scale=None, geometry_offset: int = 0,
                        capacity: int | None = None, out=None, accumulate: bool = False, first_row: int | None = None):
        """
        ``okx_ensemble_screen``: per GEOMETRY of a column table in HBM, whether it meets every limit at every step
        (``flags``), its worst margin in units of ``scale`` and the entry that holds it; per ensemble the tally, the blame
        counts and the ascending list of the geometries that pass.  ``values`` and ``status`` as ``select_ensemble`` takes them
        (unit column stride; strided rows and a strided status byte are passed on, nothing is copied).  Returns an
        ``EnsembleScreening`` of device tensors - ``margin`` and ``pass_index`` stay in HBM for whatever follows -;
        ``.finalize()`` copies it to the host (``ensemble_stats.EnsembleScreen``).  ``out``: the screening of an earlier call or
        of ``screen_prepare`` - it carries its own limits and scale; with it and a table shape seen before, the call uploads
        and allocates nothing and is legal inside a stream capture.  ``accumulate=True`` (with ``out``) adds this chunk to
        what ``out`` holds: tally and blame add and the survivors are appended.  The call's per-geometry verdicts are written
        from row ``first_row`` of ``out``'s tables on (None: ``geometry_offset`` with ``out=``, else 0).  Bit-identical from
        run to run.
        """
        g, s, k, ld, stride = self._ensemble_table(values, status, steps_per_geometry)
        row = int(first_row) if first_row is not None else (0 if out is None else int(geometry_offset))
        if out is None and limits is None:
            raise ValueError("limits are needed (or out=, which carries its own)")
        if self._new_result(out, (limits, scale, capacity), "limits, scale and capacity", accumulate, "accumulate=True adds to out="):
            out = self.screen_prepare(s, k, limits, scale, row + g, capacity)
        if out.shape != (s, k) or out.blame.device != self.device:
            raise ValueError(f"out was prepared for [S, K] = {list(out.shape)} on {out.blame.device}")
        rows = (_rows(out.flags),)
        self._check_tables("out must hold contiguous device tables limits [S, K, 2], scale [S, K], flags [G], margin [G], entry [G], tally [4], "
                           "blame [S, K, 2], pass_index [capacity] and pass_count [1]",
                           [(out.limits, (s, k, 2), F64), (out.flags, rows, U8), (out.margin, rows, F64), (out.entry, rows, I32), (out.tally, (4,), I64),
                            (out.blame, (s, k, 2), I64), (out.pass_index, (_rows(out.pass_index),), I64), (out.pass_count, (1,), I64)],
                           [(out.scale, (s, k), F64)])
        if row < 0 or row + g > out.flags.shape[0]:
            raise ValueError(f"out holds {out.flags.shape[0]} geometries: rows [{row}, {row + g}) do not fit")
        scratch = self._ensemble_scratch("screen", int(self.lib.okx_ensemble_screen_scratch_bytes(g, s, k)))
        self._ensemble_call("okx_ensemble_screen", g, s, k, _ptr(values), ld, _ptr(status), stride, _ptr(out.limits), _ptr(out.scale),
                            int(geometry_offset), 1 if accumulate else 0, _ptr(out.flags, row), _ptr(out.margin, row), _ptr(out.entry, row),
                            _ptr(out.tally), _ptr(out.blame), _ptr(out.pass_index), out.pass_index.shape[0], _ptr(out.pass_count),
                            _ptr(scratch), scratch.numel())
        return out

    # ---- okx_ensemble_covariance: Gram matrix and sums of selected entries over the complete cases (ensemble_stats) ----

    def covariance_ensemble(self, values, *, steps_per_geometry: int, status=None, entries=None, shift=None, out=None, accumulate: bool = False):
        """
        ``okx_ensemble_covariance``: the covariance accumulator (``ensemble_stats.CovarianceAccumulator``, device tensors:
        ``gram [N, N]``, ``sum [N]``, ``counts [2]`` = used, dropped, ``used [G]`` uint8) of ``entries`` - N distinct indices
        ``s K + k`` in the order wanted for rows and columns, None: all ``S K`` - of a column table in HBM over its COMPLETE
        geometries, those whose every selected entry counts.  ``values`` and ``status`` as ``reduce_ensemble`` takes them (unit
        column stride; strided rows and a strided status byte are passed on, nothing is copied); ``shift [S, K]`` the common
        shift (None: the table's own geometry 0, undefined entries 0 - chunks that are accumulated need ONE shift, pass it
        or pass ``out=``).  ``out``: the accumulator of an earlier call - it carries its own shift and entries - to write
        (``accumulate=False``) or add into (``True``); with it and a table shape seen before, the call uploads and allocates
        nothing and is legal inside a stream capture (``out.used`` is written when it holds a byte per geometry of the call).
        ``.finalize()`` copies to the host: mean, covariance, std, correlation.  Bit-identical from run to run; different
        chunkings agree to rounding.
        """
        g, s, k, ld, stride = self._ensemble_table(values, status, steps_per_geometry)
        dev = self.device
        if self._new_result(out, (shift, entries), "shift and entries", accumulate):
            host = None if entries is None else np.ascontiguousarray(check_covariance_arguments(
                entries.detach().cpu().numpy() if isinstance(entries, torch.Tensor) else entries, s * k))
            n = s * k if host is None else host.size
            rc = self.lib.okx_ensemble_covariance_check(None if host is None else host.ctypes.data_as(C.c_void_p), min(n, 1 << 30), s * k)
            _lib.check(rc, "okx_ensemble_covariance")
            shift = self._ensemble_shift(shift, values, g, s, k)
            index = torch.arange(n, dtype=torch.int32, device=dev) if host is None else torch.as_tensor(host, device=dev)
            out = CovarianceAccumulator(torch.empty((n, n), dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev),
                                        torch.empty(2, dtype=torch.int64, device=dev), shift, index, torch.empty(g, dtype=torch.uint8, device=dev),
                                        natural=host is None)  # (all entries in natural order: the call passes no entry list)
        n = _rows(out.entries)
        self._check_tables(f"out must hold contiguous device tables gram [N, N], sum [N], counts [2], entries [N] and shift [S, K] = [{s}, {k}]",
                           [(out.gram, (n, n), F64), (out.sum, (n,), F64), (out.counts, (2,), I64), (out.shift, (s, k), F64), (out.entries, (n,), I32)])
        used = out.used  # (written when it holds a byte per geometry of the call)
        if used is not None and (used.dtype != U8 or used.shape[0] < g or not used.is_contiguous() or used.device != dev):
            used = None
        scratch = self._ensemble_scratch("covariance", int(self.lib.okx_ensemble_covariance_scratch_bytes(g, s, k, n)))
        index = None if out.natural and n == s * k else _ptr(out.entries)
        self._ensemble_call("okx_ensemble_covariance", g, s, k, _ptr(values), ld, _ptr(status), stride, index, n, _ptr(out.shift),
                            1 if accumulate else 0, _ptr(out.gram), _ptr(out.sum), _ptr(out.counts), _ptr(used), _ptr(scratch), scratch.numel())
        return out

    # ---- okx_ensemble_curves: the characteristics of every geometry's curves along the sweep (ensemble_stats.EnsembleCurves) ----

    def curves_prepare(self, steps: int, n_columns: int, n_geometries: int, *, abscissa, scale, origin=0.0, degree: int = 2, window=None):
        """
        The tables of a curves pass over ``[steps, n_columns]`` entries and ``n_geometries`` geometries: the arguments are
        validated (``okx_ensemble_curves_check``), a shared abscissa ``[S]`` is uploaded ONCE (an integer ``abscissa`` names a
        column of the table) and ``features [G, K, 12]`` / ``count [G, K]`` are allocated.
        """
        s, k, g = int(steps), int(n_columns), int(n_geometries)
        if g < 0:
            raise ValueError("negative geometry count")
        shared = None
        if abscissa is None:
            raise ValueError("abscissa is needed: a column of the table or a shared [S] table (or out=, which carries its own)")
        if isinstance(abscissa, (int, np.integer)) and not isinstance(abscissa, bool):
            kx, n_x = int(abscissa), -1
        else:
            shared = np.ascontiguousarray(_host_f64(abscissa).reshape(-1))
            kx, n_x = 0, shared.size
        degree = int(degree) if not isinstance(degree, bool) and int(degree) == degree else -1
        lo, hi = (-np.inf, np.inf) if window is None else (float(window[0]), float(window[1]))
        rc = self.lib.okx_ensemble_curves_check(s, k, n_x, kx, float(origin), float(scale), lo, hi, degree)
        _lib.check(rc, "okx_ensemble_curves")
        dev = self.device
        return EnsembleCurves(torch.empty((g, k, CURVE_FIELDS), dtype=torch.float64, device=dev), torch.empty((g, k), dtype=torch.int32, device=dev),
                              None if shared is None else torch.as_tensor(shared, device=dev),
                              (kx if shared is None else -1, float(origin), float(scale), lo, hi, degree))

    def curves_ensemble(self, values, *, steps_per_geometry: int, abscissa=None, scale=None, status=None, origin=None, degree=None,
                        window=None, out=None, first_row: int = 0):
        """
        ``okx_ensemble_curves``: per GEOMETRY and column of a column table in HBM, the characteristics of the curve along the
        sweep - the least-squares polynomial of ``degree`` (0 .. 3, default 2) in ``u = (x - origin) / scale`` over the used
        steps, its residuals, the extremes and where they occur (``ensemble_stats.EnsembleCurves`` of device tensors:
        ``features [G, K, 12]``, ``count [G, K]`` int32).  ``abscissa``: a shared ``x [S]`` or an integer column of the table
        (every geometry against its own ``wheel_travel``); ``window = (lo, hi)`` in x units, closed.  ``values`` and ``status``
        as ``screen_ensemble`` takes them (unit column stride; strided rows and a strided status byte are passed on, nothing
        is copied).  ``.table()`` is the ``[G, K * 12]`` column table the other passes take with ``steps_per_geometry=1``;
        ``.finalize()`` copies to the host.  ``out``: the curves of an earlier call or of ``curves_prepare`` - it carries its
        own arguments; with it and a table shape seen before, the call uploads and allocates nothing and is legal inside a
        stream capture.  The call's geometries are written from row ``first_row`` of ``out``'s tables on.  A geometry's
        features depend on its own rows alone: bit-identical from run to run and however the geometries are chunked.
        """
        g, s, k, ld, stride = self._ensemble_table(values, status, steps_per_geometry)
        row = int(first_row)
        if self._new_result(out, (abscissa, scale, origin, degree, window), "abscissa, origin, scale, degree and window"):
            if scale is None:
                raise ValueError("abscissa and scale are needed (or out=, which carries its own)")
            out = self.curves_prepare(s, k, row + g, abscissa=abscissa, scale=scale, origin=0.0 if origin is None else origin,
                                      degree=2 if degree is None else degree, window=window)
        f, n = out.features, out.count
        rows = _rows(f)
        self._check_tables(f"out must hold contiguous device tables features [G, {k}, 12] and count [G, {k}]",
                           [(f, (rows, k, CURVE_FIELDS), F64), (n, (rows, k), I32)], [(out.abscissa, (_rows(out.abscissa),), F64)])
        if out.abscissa is not None and out.abscissa.shape[0] != s:
            raise ValueError(f"out was prepared for {out.abscissa.shape[0]} steps")
        if row < 0 or row + g > f.shape[0]:
            raise ValueError(f"out holds {f.shape[0]} geometries: rows [{row}, {row + g}) do not fit")
        kx, origin, scale, lo, hi, degree = out.arguments
        self._ensemble_call("okx_ensemble_curves", g, s, k, _ptr(values), ld, _ptr(status), stride, _ptr(out.abscissa), max(kx, 0), origin, scale,
                            lo, hi, degree, _ptr(f, row), _ptr(n, row))
        return out

    # ---- okx_ensemble_front: the nondominated (Pareto) front of the ensemble on up to 8 objectives (ensemble_stats.EnsembleFront) ----

    def front_prepare(self, steps: int, n_columns: int, n_geometries: int, objectives, capacity: int | None = None) -> "EnsembleFronting":
        """
        The tables of a front pass over ``[steps, n_columns]`` entries and ``n_geometries`` geometries: ``objectives`` - a
        sequence of ``(step, column, sense)`` or ``(step, column, "target", value)`` - are validated
        (``okx_ensemble_front_check``) and kept as the host arrays every launch reads; ``dominated [G]``, ``tally [3]`` and the
        front list with ``capacity`` slots (None: one per geometry) are allocated.
        """
        s, k, g = int(steps), int(n_columns), int(n_geometries)
        if g < 0 or (capacity is not None and int(capacity) < 0):
            raise ValueError("negative geometry count or capacity")
        entries, sense, target = check_front_arguments(objectives, s, k, g)
        rc = self.lib.okx_ensemble_front_check(g, s, k, entries.ctypes.data_as(C.c_void_p), sense.ctypes.data_as(C.c_void_p),
                                               target.ctypes.data_as(C.c_void_p), entries.size)
        _lib.check(rc, "okx_ensemble_front")
        dev, cap = self.device, g if capacity is None else int(capacity)
        return EnsembleFronting(self, entries, sense, target, torch.empty(g, dtype=torch.int32, device=dev), torch.zeros(3, dtype=torch.int64, device=dev),
                                torch.empty(cap, dtype=torch.int64, device=dev), torch.empty((cap, entries.size), dtype=torch.float64, device=dev))

    def front_ensemble(self, values, *, steps_per_geometry: int, objectives=None, status=None, mask=None, index=None, geometry_offset: int = 0,
                       capacity: int | None = None, out=None):
        """
        ``okx_ensemble_front``: which geometries of a column table in HBM no other geometry beats on every objective at once.
        ``objectives``: up to 8 of ``(step, column, "min" | "max")`` or ``(step, column, "target", value)``; ``values`` and
        ``status`` as ``screen_ensemble`` takes them; ``mask [G]`` uint8 (may be strided), 0: the geometry may be a candidate -
        ``screen_ensemble``'s ``flags`` as they lie in HBM -; ``index [G]`` int64 the ids of the geometries (None:
        ``geometry_offset + g``).  Returns an ``EnsembleFronting`` of device tensors: ``dominated [G]`` (how many candidates
        dominate the geometry, -1: no candidate, 0: on the front), ``tally [3]``, ``front_index [capacity]`` and ``front_values
        [capacity, M]`` (``capacity`` defaults to the geometry count); ``.finalize()`` makes the only host read and raises if
        the front was truncated; ``.merge(other)`` is the front of two runs' union.  ``out``: the run of an earlier call or of
        ``front_prepare`` - it carries its own objectives and capacity; with it and a table shape seen before, the call
        allocates nothing and is legal inside a stream capture.  Only comparisons: exact, and bit-identical from run to run.
        """
        g, s, k, ld, stride = self._ensemble_table(values, status, steps_per_geometry)
        if self._new_result(out, (objectives, capacity), "objectives and capacity"):
            if objectives is None:
                raise ValueError("objectives are needed (or out=, which carries its own)")
            out = self.front_prepare(s, k, g, objectives, capacity)
        dev = self.device
        if out.dominated is None or out.dominated.shape[0] < g or out.tally.device != dev:
            raise ValueError(f"out holds no dominated table for {g} geometries on {dev}")
        m = int(out.entries.size)
        capacity = _rows(out.front_index)
        self._check_tables(f"out must hold contiguous device tables dominated [G], tally [3], front_index [capacity] and front_values [capacity, {m}]",
                           [(out.dominated, (_rows(out.dominated),), I32), (out.tally, (3,), I64), (out.front_index, (capacity,), I64),
                            (out.front_values, (capacity, m), F64)])
        mask_stride = self._check_mask(mask, g, contiguous=False)
        if index is not None and (index.dtype != torch.int64 or index.dim() != 1 or index.shape[0] != g or index.device != dev or not index.is_contiguous()):
            raise ValueError("index must be a contiguous int64 [G] device tensor")
        scratch = self._ensemble_scratch("front", int(self.lib.okx_ensemble_front_scratch_bytes(g, m)))
        self._ensemble_call("okx_ensemble_front", g, s, k, _ptr(values), ld, _ptr(status), stride, out.entries.ctypes.data_as(C.c_void_p),
                            out.sense.ctypes.data_as(C.c_void_p), out.target.ctypes.data_as(C.c_void_p), m, _ptr(mask), mask_stride, _ptr(index),
                            int(geometry_offset), _ptr(out.dominated), _ptr(out.tally), _ptr(out.front_index), _ptr(out.front_values), out.capacity,
                            _ptr(scratch), scratch.numel())
        return out

    # ---- okx_ensemble_sample: the hardpoint table of a plan's ensemble, drawn on device (ensemble_sample.SamplePlan) ----

    def _plan_tables(self, plan, build) -> dict:
        """``build(plan)``, made ONCE per plan object: the entry is keyed by ``id(plan)``, guarded by a weak reference (an id may be
        reused) and dropped when the plan dies."""
        plans, key = self.__dict__.setdefault("_sample_plans", {}), id(plan)
        held = plans.get(key)
        if held is not None and held[0]() is plan:
            return held[1]
        tables = build(plan)
        plans[key] = (weakref.ref(plan, lambda r: plans.pop(key, None) if plans.get(key, (None,))[0] is r else None), tables)
        return tables

    def _sample_tables(self, plan) -> dict:
        """The plan's tables on the device and its guards as the host array a launch reads, validated (``okx_ensemble_sample_check``)
        and uploaded ONCE per plan.  They are held for as long as the plan object lives and dropped with it (a search loop makes a
        plan per generation); whoever keeps a captured graph of a launch keeps its plan."""
        def build(plan):
            ints, reals = plan.guard_table()
            guards = (SampleGuard * max(1, len(plan.guards)))()
            for i in range(len(plan.guards)):
                guards[i] = SampleGuard(*(int(v) for v in ints[i]), float(reals[i, 0]), float(reals[i, 1]))
            rc = self.lib.okx_ensemble_sample_check(0, 0, plan.n_total, plan.n_points, plan.coords.ctypes.data_as(C.c_void_p), plan.n_coords,
                                                    plan.kind.ctypes.data_as(C.c_void_p), plan.bound.ctypes.data_as(C.c_void_p), plan.n_latents,
                                                    0 if plan.mixing is None else 1, guards, len(plan.guards), plan.stratify, plan.max_attempts)
            _lib.check(rc, "okx_ensemble_sample")
            up = lambda a: None if a is None else torch.tensor(np.asarray(a), device=self.device)  # noqa: E731
            return dict(nominal=up(plan.nominal), coords=up(plan.coords), kind=up(plan.kind), bound=up(plan.bound_table()), mixing=up(plan.mixing),
                        scale=up(plan.scale), guards=guards)

        return self._plan_tables(plan, build)

    def _family_tables(self, fplan) -> dict:
        """The wrapped plan's tables (``_sample_tables``) and the group table on the device, validated
        (``okx_ensemble_sample_families_check``) and uploaded ONCE per plan object; dropped with it."""
        def build(fplan):
            plan = fplan.plan
            tables = dict(self._sample_tables(plan))
            rc = self.lib.okx_ensemble_sample_families_check(0, 0, fplan.n_families, plan.n_points, plan.coords.ctypes.data_as(C.c_void_p), plan.n_coords,
                                                             plan.kind.ctypes.data_as(C.c_void_p), plan.bound.ctypes.data_as(C.c_void_p), plan.n_latents,
                                                             0 if plan.mixing is None else 1, fplan.group.ctypes.data_as(C.c_void_p), fplan.n_groups,
                                                             tables["guards"], len(plan.guards), plan.stratify, plan.max_attempts)
            _lib.check(rc, "okx_ensemble_sample_families")
            tables["group"] = torch.tensor(np.asarray(fplan.group), device=self.device)
            return tables

        return self._plan_tables(fplan, build)

    def _sample_out(self, who: str, plan, base, lo, hi, latents: bool, delta: bool, out) -> tuple:
        """``(n, lo, out)`` of a draw of geometries ``[lo, hi)`` of ``plan`` (``base``: the ``SamplePlan`` that sets the table shapes):
        the range checked, the ``EnsembleSample`` made or - ``out=`` - its tables checked, and ``out.lo`` set."""
        lo = int(lo)
        hi = int(plan.n_total) if hi is None else int(hi)
        n = hi - lo
        if n < 0 or lo < 0:
            raise ValueError(f"{who}: bad range [{lo}, {hi})")
        dev, p, f, z = self.device, base.n_points, base.n_coords, base.n_latents
        if out is None:
            return n, lo, EnsembleSample(torch.empty((n, p, 3), dtype=F64, device=dev), torch.empty((n, z), dtype=F64, device=dev) if latents else None,
                                         torch.empty((n, f), dtype=F64, device=dev) if delta else None, torch.empty(n, dtype=U8, device=dev), lo)
        self._check_tables(f"out must hold contiguous device tables hardpoints [{n}, {p}, 3], latents [{n}, {z}], delta [{n}, {f}] and flags [{n}]", [],
                           [(out.hardpoints, (n, p, 3), F64), (out.latents, (n, z), F64), (out.delta, (n, f), F64), (out.flags, (n,), U8)])
        if out.hardpoints is None:
            raise ValueError("out holds no hardpoint table")
        out.lo = lo
        return n, lo, out

    def sample_ensemble(self, plan, lo: int = 0, hi: int | None = None, *, latents: bool = False, delta: bool = False, out=None) -> "EnsembleSample":
        """
        ``okx_ensemble_sample``: geometries ``[lo, hi)`` (``hi`` None: ``plan.n_total``) of the ensemble of ``plan``
        (``ensemble_sample.SamplePlan``), drawn in HBM - the bits of ``ensemble_sample.sample_host(plan, lo, hi)``, whatever the
        range is cut into and wherever it is drawn.  Returns an ``EnsembleSample`` of device tensors; ``latents`` / ``delta`` ask for
        those tables too.  ``out``: the ``EnsembleSample`` of an earlier call of the same shape to write into - with it (and a
        plan seen before) the call allocates nothing and is legal inside a stream capture.
        """
        n, lo, out = self._sample_out("okx_ensemble_sample", plan, plan, lo, hi, latents, delta, out)
        t = self._sample_tables(plan)
        self._ensemble_call("okx_ensemble_sample", n, lo, int(plan.n_total), C.c_uint64(plan.seed), plan.n_points, _ptr(t["nominal"]), _ptr(t["coords"]),
                            plan.n_coords, _ptr(t["kind"]), _ptr(t["bound"]), plan.n_latents, _ptr(t["mixing"]), _ptr(t["scale"]), t["guards"],
                            len(plan.guards), plan.stratify, plan.max_attempts, _ptr(out.hardpoints), _ptr(out.latents), _ptr(out.delta), _ptr(out.flags))
        return out

    # ---- okx_ensemble_sample_families: the pick-freeze ensemble of a FamilyPlan, drawn on device (ensemble_sample.FamilyPlan) ----

    def sample_families(self, plan, lo: int = 0, hi: int | None = None, *, latents: bool = False, delta: bool = False, out=None) -> "EnsembleSample":
        """
        ``okx_ensemble_sample_families``: geometries ``[lo, hi)`` (``hi`` None: ``plan.n_total = n_families * M``) of the pick-freeze
        ensemble of ``plan`` (``ensemble_sample.FamilyPlan``), drawn in HBM - the bits of ``ensemble_sample.families_host(plan, lo, hi)``,
        whatever the range is cut into (family-aligned or not) and wherever it is drawn.  Returns an ``EnsembleSample`` of device
        tensors; ``flags`` is 1 where a guard fails (the ``mask`` of ``sobol_ensemble``).  ``out``: the ``EnsembleSample`` of an earlier
        call of the same shape - with it (and a plan seen before) the call allocates nothing and is legal inside a stream capture.
        """
        base = plan.plan
        n, lo, out = self._sample_out("okx_ensemble_sample_families", plan, base, lo, hi, latents, delta, out)
        t = self._family_tables(plan)
        self._ensemble_call("okx_ensemble_sample_families", n, lo, int(plan.n_families), C.c_uint64(base.seed), base.n_points, _ptr(t["nominal"]),
                            _ptr(t["coords"]), base.n_coords, _ptr(t["kind"]), _ptr(t["bound"]), base.n_latents, _ptr(t["mixing"]), _ptr(t["scale"]),
                            _ptr(t["group"]), int(plan.n_groups), t["guards"], len(base.guards), base.stratify, _ptr(out.hardpoints),
                            _ptr(out.latents), _ptr(out.delta), _ptr(out.flags))
        return out

    # ---- okx_ensemble_sobol: the variance decomposition of an evaluated pick-freeze ensemble (ensemble_stats.EnsembleSobol) ----

    def sobol_ensemble(self, values, *, steps_per_geometry: int, n_groups: int, status=None, mask=None, shift=None, out=None, accumulate: bool = False,
                       group_names=None):
        """
        ``okx_ensemble_sobol``: the Sobol' accumulator (``ensemble_stats.SobolAccumulator``, device tensors: ``acc [S, K, 6 + 3 D]``,
        ``shift [S, K]``) of a column table in HBM whose geometries are the families of ``sample_families`` - ``M = n_groups + 2``
        consecutive geometries each.  ``values`` and ``status`` as ``reduce_ensemble`` takes them (unit column stride; strided rows and
        a strided status byte are passed on, nothing is copied); ``mask [G]`` contiguous uint8, bit 0 set: the member does not
        count - the sampler's ``flags`` as they lie in HBM; a family counts at an entry when all its members do.  ``shift [S, K]``
        the common shift (None: the table's own geometry 0, undefined entries 0 - chunks that are accumulated need ONE shift,
        pass it or pass ``out=``).  ``out``: the accumulator of an earlier call - it carries its own shift - to write
        (``accumulate=False``) or add into (``True``); with it and a table shape seen before, the call allocates nothing and is
        legal inside a stream capture.  ``.finalize()`` copies to the host: first-order and total-order indices per group.
        Bit-identical from run to run; different chunkings agree to rounding, exactly when the sums are exact.
        """
        g, s, k, ld, stride = self._ensemble_table(values, status, steps_per_geometry)
        d = int(n_groups)
        n, out = self._sobol_out("okx_ensemble_sobol", (g, s, k), d, 0, mask, shift, values, out, accumulate, (s, k, SOBOL_FIELDS + 3 * d),
                                 f"out must hold contiguous device tables acc [S, K, {SOBOL_FIELDS + 3 * d}] and shift [S, K] = [{s}, {k}]",
                                 lambda acc, shift: SobolAccumulator(acc, shift, group_names))
        scratch = self._ensemble_scratch("sobol", int(self.lib.okx_ensemble_sobol_scratch_bytes(n, d, s, k)))
        self._ensemble_call("okx_ensemble_sobol", n, d, s, k, _ptr(values), ld, _ptr(status), stride, _ptr(mask), _ptr(out.shift),
                            1 if accumulate else 0, _ptr(out.acc), _ptr(scratch), scratch.numel())
        return out

    def _sobol_out(self, who: str, table: tuple, d: int, family_offset: int, mask, shift, values, out, accumulate: bool, acc_shape: tuple, message: str,
                   new) -> tuple:
        """The front end ``sobol_ensemble`` and ``sobol_bootstrap_ensemble`` share: the group count, whole families, the accumulator
        - ``new(acc, shift)`` or ``out=``, its tables checked (``message``) - and the mask.  Returns ``(families, out)``."""
        g, s, k = table
        if not 1 <= d <= SOBOL_MAX_GROUPS:
            raise ValueError(f"{who}: {d} groups, 1 to {SOBOL_MAX_GROUPS} allowed")
        if g % (d + 2):
            raise ValueError(f"{who}: {g} geometries are no whole families of {d + 2}")
        if family_offset < 0:
            raise ValueError(f"{who}: negative family_offset")
        if self._new_result(out, (shift,), "shift", accumulate):
            out = new(torch.empty(acc_shape, dtype=F64, device=self.device), self._ensemble_shift(shift, values, g, s, k))
        self._check_tables(message, [(out.acc, acc_shape, F64), (out.shift, (s, k), F64)])
        self._check_mask(mask, g, contiguous=True)
        return g // (d + 2), out

    # ---- okx_ensemble_bootstrap_weights / okx_ensemble_sobol_bootstrap: how far to trust the indices (ensemble_stats.EnsembleSobolBootstrap) ----

    def bootstrap_weights(self, n_rows: int, n_replicates: int, seed: int, row_offset: int = 0, out=None) -> torch.Tensor:
        """
        ``okx_ensemble_bootstrap_weights``: the Poisson(1) bootstrap weights ``uint8 [n_rows, R]`` of GLOBAL rows
        ``[row_offset, row_offset + n_rows)`` in HBM - the bytes of ``ensemble_stats.bootstrap_weights(seed, row_offset, row_offset + n_rows, R)``,
        a pure function of ``(seed, row, replicate)`` wherever and in whatever ranges they are drawn.  ``out``: the tensor of an earlier
        call of the same shape (then the call allocates nothing and is legal inside a stream capture).
        """
        n, r, lo = int(n_rows), check_replicates("okx_ensemble_bootstrap_weights", n_replicates), int(row_offset)
        if n < 0 or lo < 0:
            raise ValueError(f"okx_ensemble_bootstrap_weights: bad range [{lo}, {lo + n})")
        if out is None:
            out = torch.empty((n, r), dtype=U8, device=self.device)
        self._check_tables(f"out must be a contiguous uint8 [{n}, {r}] device tensor", [(out, (n, r), U8)])
        self._ensemble_call("okx_ensemble_bootstrap_weights", n, lo, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), r, _ptr(out))
        return out

    def sobol_bootstrap_ensemble(self, values, *, steps_per_geometry: int, n_groups: int, n_replicates: int, seed: int, family_offset: int = 0,
                                 status=None, mask=None, shift=None, out=None, accumulate: bool = False, group_names=None):
        """
        ``okx_ensemble_sobol_bootstrap``: ``n_replicates`` Poisson-bootstrap replicates of the Sobol' accumulator of ``sobol_ensemble`` over
        the same table (``ensemble_stats.SobolBootstrapAccumulator``, device tensors: ``acc [R, S, K, 6 + 3 D]``, ``shift [S, K]``) - replicate
        ``r`` weighs family ``i`` of the table, GLOBAL family ``family_offset + i``, with ``bootstrap_weights(...)[i, r]`` of ``seed``.
        ``values``, ``status``, ``mask``, ``shift``, ``out`` and ``accumulate`` as ``sobol_ensemble`` takes them; chunks that are accumulated
        pass their ``family_offset`` (and ONE shift and seed: ``out=`` carries both).  ``.finalize(level)`` copies to the host: the
        replicates' indices, their standard deviations and percentile intervals.  Bit-identical from run to run; different chunkings
        agree to rounding, exactly when the sums are exact.
        """
        who = "okx_ensemble_sobol_bootstrap"
        g, s, k, ld, stride = self._ensemble_table(values, status, steps_per_geometry)
        d, r, first, seed = int(n_groups), check_replicates(who, n_replicates), int(family_offset), int(seed) & 0xFFFFFFFFFFFFFFFF
        n, out = self._sobol_out(who, (g, s, k), d, first, mask, shift, values, out, accumulate, (r, s, k, SOBOL_FIELDS + 3 * d),
                                 f"out must hold contiguous device tables acc [R, S, K, {SOBOL_FIELDS + 3 * d}] = [{r}, {s}, {k}, .] and shift [S, K]",
                                 lambda acc, shift: SobolBootstrapAccumulator(acc, shift, seed, group_names))
        if out.seed != seed:
            raise ValueError(f"out= was taken with seed {out.seed}, not {seed}")
        scratch = self._ensemble_scratch("sobol_bootstrap", int(self.lib.okx_ensemble_sobol_bootstrap_scratch_bytes(n, d, s, k, r)))
        self._ensemble_call(who, n, first, d, s, k, _ptr(values), ld, _ptr(status), stride, _ptr(mask), _ptr(out.shift), C.c_uint64(seed), r,
                            1 if accumulate else 0, _ptr(out.acc), _ptr(scratch), scratch.numel())
        return out

    # ---- okx_ensemble_bin / okx_ensemble_effects: conditional moments over the bins of every factor (ensemble_stats.EnsembleEffects) ----

    def bin_factors(self, factors, edges=None, out=None) -> "EffectBins":
        """
        ``okx_ensemble_bin``: the bins of ``factors [G, F]`` (a float64 device tensor with unit column stride; rows may be strided) against
        ``edges [F, B - 1]`` - ``ensemble_stats.effects_edges``; validated on the host (finite, non-decreasing) and uploaded - as an
        ``EffectBins`` of device tensors: the bin bytes, per factor the list of its geometries bin by bin and where every bin starts.
        Done ONCE for an ensemble: factors do not change from step to step.  ``out``: the ``EffectBins`` of an earlier call of the same
        shape - it carries its own edges; with it the call uploads and allocates nothing and is legal inside a stream capture.
        Integers and comparisons only: the bytes of ``ensemble_stats.bin_factors_host`` / ``bin_lists_host``, the same every run.
        """
        dev = self.device
        if not isinstance(factors, torch.Tensor) or factors.dim() != 2 or factors.dtype != F64 or factors.device != dev \
                or (factors.shape[1] > 1 and factors.stride(1) != 1):
            raise ValueError("factors must be a float64 [G, F] device tensor with unit column stride")
        g, f = factors.shape
        ldf = factors.stride(0) if g > 1 else max(f, factors.stride(0))
        if ldf < f:
            raise ValueError("rows of factors overlap")
        if self._new_result(out, (edges,), "edges"):
            if edges is None:
                raise ValueError("edges are needed (or out=, which carries its own)")
            host = _host_f64(edges)
            b = host.shape[1] + 1 if host.ndim == 2 else 0
            b, host, _ = check_effects_arguments(b, f, host)
            out = EffectBins(torch.empty((g, f), dtype=U8, device=dev), torch.empty((f, g), dtype=I32, device=dev),
                             torch.empty((f, b + 1), dtype=I64, device=dev), torch.as_tensor(host, device=dev), b)
        b = int(out.n_bins)
        self._check_tables(f"out must hold contiguous device tables bins [{g}, {f}], order [{f}, {g}], offsets [{f}, {b + 1}] and edges [{f}, {b - 1}]",
                           [(out.bins, (g, f), U8), (out.order, (f, g), I32), (out.offsets, (f, b + 1), I64), (out.edges, (f, b - 1), F64)])
        self._ensemble_call("okx_ensemble_bin", g, f, _ptr(factors), ldf, _ptr(out.edges), b, _ptr(out.bins), _ptr(out.order), _ptr(out.offsets))
        return out

    def effects_ensemble(self, values, *, steps_per_geometry: int, bins, status=None, mask=None, shift=None, out=None, accumulate: bool = False,
                         factor_names=None):
        """
        ``okx_ensemble_effects``: the main-effects accumulator (``ensemble_stats.EffectsAccumulator``, device tensors: ``acc [F, B, 3, S, K]``
        = count, sum d, sum d^2 of every bin of every factor, ``shift [S, K]``, ``edges [F, B - 1]``) of a column table in HBM.  ``values``
        and ``status`` as ``reduce_ensemble`` takes them (unit column stride; strided rows and a strided status byte are passed on,
        nothing is copied); ``bins``: the ``EffectBins`` ``bin_factors`` made of the factors of THESE geometries; ``mask [G]`` contiguous
        uint8, bit 0 set: the geometry does not count - the sampler's ``flags`` as they lie in HBM.  ``shift [S, K]`` the common shift
        (None: the table's own geometry 0, undefined entries 0 - chunks that are accumulated need ONE shift, pass it or pass
        ``out=``).  ``out``: the accumulator of an earlier call - it carries its own shift - to write (``accumulate=False``) or to go on
        from (``True``); with it and a table shape seen before, the call allocates nothing and is legal inside a stream capture.
        ``.finalize()`` copies to the host: conditional means, within-bin spreads, first-order indices.  Every cell is one chain of
        additions in ascending geometry order: bit-identical from run to run, and chunks accumulated in ascending order carry the
        bits of the whole table.
        """
        g, s, k, ld, stride = self._ensemble_table(values, status, steps_per_geometry)
        if not isinstance(bins, EffectBins):
            raise ValueError("bins must be the EffectBins of bin_factors")
        f, b = _rows(bins.order), int(bins.n_bins)
        self._check_tables(f"bins must hold contiguous device tables order [F, {g}] and offsets [F, {b + 1}] of the table's {g} geometries",
                           [(bins.order, (f, g), I32), (bins.offsets, (f, b + 1), I64), (bins.edges, (f, b - 1), F64)])
        if self._new_result(out, (shift,), "shift", accumulate):
            out = EffectsAccumulator(torch.empty((f, b, EFFECTS_FIELDS, s, k), dtype=F64, device=self.device), self._ensemble_shift(shift, values, g, s, k),
                                     bins.edges, factor_names)
        self._check_tables(f"out must hold contiguous device tables acc [{f}, {b}, {EFFECTS_FIELDS}, S, K], shift [S, K] = [{s}, {k}] and edges [{f}, {b - 1}]",
                           [(out.acc, (f, b, EFFECTS_FIELDS, s, k), F64), (out.shift, (s, k), F64), (out.edges, (f, b - 1), F64)])
        self._check_mask(mask, g, contiguous=True)
        self._ensemble_call("okx_ensemble_effects", g, s, k, _ptr(values), ld, _ptr(status), stride, _ptr(mask), f, b, _ptr(bins.order), _ptr(bins.offsets),
                            _ptr(out.shift), 1 if accumulate else 0, _ptr(out.acc))
        return out

    # ---- okx_ensemble_tilt_weights / okx_ensemble_reweigh: tolerance what-ifs by likelihood reweighting (ensemble_stats.EnsembleWhatIf) ----

    def tilt_prepare(self, scenarios) -> torch.Tensor:
        """
        The scenario table ``[N, Z, 5]`` of ``ensemble_sample.tolerance_scenarios`` validated on the host (``okx_ensemble_tilt_check``: no NaN,
        ``lo <= hi``, finite ``a, b, c``, the caps) and uploaded ONCE: the float64 device tensor ``tilt_weights`` takes.
        """
        host = np.ascontiguousarray(_host_f64(scenarios))
        if host.ndim != 3 or host.shape[2] != 5:
            raise ValueError("scenarios must be the [N, Z, 5] table of ensemble_sample.tolerance_scenarios")
        rc = self.lib.okx_ensemble_tilt_check(host.ctypes.data_as(C.c_void_p), min(host.shape[0], REWEIGH_MAX_SCENARIOS + 1), min(host.shape[1], 1 << 20))
        _lib.check(rc, "okx_ensemble_tilt_weights")
        return torch.as_tensor(host, device=self.device)

    def tilt_weights(self, latents, scenarios, out=None) -> torch.Tensor:
        """
        ``okx_ensemble_tilt_weights``: the likelihood ratios ``float64 [G, N]`` of the geometries whose latents are ``latents [G, Z]`` (a
        float64 device tensor with unit column stride; rows may be strided - the sampler's ``latents`` as they lie in HBM) under the ``N``
        scenarios of ``scenarios``: the table of ``ensemble_sample.tolerance_scenarios`` (validated and uploaded by this call) or the device
        tensor ``tilt_prepare`` made of it (then the call uploads nothing).  The bits of ``ensemble_sample.tilt_weights_host``.  ``out``: a
        ``[G, N]`` float64 device tensor with unit column stride to write into (rows may be strided); with it and a prepared table the call
        allocates nothing and is legal inside a stream capture.
        """
        dev = self.device
        if not isinstance(latents, torch.Tensor) or latents.dim() != 2 or latents.dtype != F64 or latents.device != dev \
                or (latents.shape[1] > 1 and latents.stride(1) != 1):
            raise ValueError("latents must be a float64 [G, Z] device tensor with unit column stride")
        g, z = latents.shape
        ldz = latents.stride(0) if g > 1 else max(z, latents.stride(0))
        if ldz < z:
            raise ValueError("rows of latents overlap")
        table = scenarios if isinstance(scenarios, torch.Tensor) and scenarios.device == dev else self.tilt_prepare(scenarios)
        n = _rows(table)
        self._check_tables(f"scenarios must be a contiguous float64 [N, {z}, 5] table, one row per latent of the table", [(table, (n, z, 5), F64)])
        if out is None:
            out = torch.empty((g, n), dtype=F64, device=dev)
        if not isinstance(out, torch.Tensor) or out.dtype != F64 or out.device != dev or tuple(out.shape) != (g, n) or (n > 1 and out.stride(1) != 1):
            raise ValueError(f"out must be a float64 [{g}, {n}] device tensor with unit column stride")
        ldw = out.stride(0) if g > 1 else max(n, out.stride(0))
        if ldw < n:
            raise ValueError("rows of out overlap")
        self._ensemble_call("okx_ensemble_tilt_weights", g, _ptr(latents), ldz, z, _ptr(table), n, _ptr(out), ldw)
        return out

    def reweigh_ensemble(self, values, *, steps_per_geometry: int, weights, status=None, mask=None, shift=None, limits=None, verdict=None, out=None,
                         accumulate: bool = False, scenario_names=None):
        """
        ``okx_ensemble_reweigh``: the what-if accumulator (``ensemble_stats.ReweighAccumulator``, device tensors: ``acc [N, 10, S, K]``,
        ``joint [N, 7]``, ``shift [S, K]``, ``limits [S, K, 2]`` or None) of a column table in HBM under ``N`` scenarios.  ``values`` and ``status``
        as ``reduce_ensemble`` takes them (unit column stride; strided rows and a strided status byte are passed on, nothing is copied);
        ``weights [G, N]`` float64 with unit column stride, what ``tilt_weights`` made of the latents of THESE geometries (or any table of
        doubles); ``mask [G]`` contiguous uint8, bit 0 set: the geometry does not count - the sampler's ``flags`` as they lie in HBM;
        ``verdict [G]`` contiguous uint8, ``screen_ensemble``'s ``flags`` (None: every geometry passes); ``limits`` ``[S, K, 2]``, ``[K, 2]`` or
        ``[2]`` = (lo, hi), validated on the host and uploaded (None: nothing is outside).  ``shift [S, K]`` the common shift (None: the table's
        own geometry 0, undefined entries 0 - chunks that are accumulated need ONE shift, pass it or pass ``out=``).  ``out``: the
        accumulator of an earlier call - it carries its own shift and limits - to write (``accumulate=False``) or add into (``True``); with
        it and a table shape seen before, the call uploads and allocates nothing and is legal inside a stream capture.  ``.finalize()``
        copies to the host: the reweighted mean, spread, effective sample size, standard errors and yields of every scenario.
        Bit-identical from run to run; different chunkings agree to rounding, exactly when the sums are exact.
        """
        g, s, k, ld, stride = self._ensemble_table(values, status, steps_per_geometry)
        dev = self.device
        if not isinstance(weights, torch.Tensor) or weights.dim() != 2 or weights.dtype != F64 or weights.device != dev or weights.shape[0] != g \
                or (weights.shape[1] > 1 and weights.stride(1) != 1):
            raise ValueError(f"weights must be a float64 [{g}, N] device tensor with unit column stride, one row per geometry of the table")
        n = int(weights.shape[1])
        if not 1 <= n <= REWEIGH_MAX_SCENARIOS:
            raise ValueError(f"okx_ensemble_reweigh: {n} scenarios, 1 to {REWEIGH_MAX_SCENARIOS} allowed")
        ldw = weights.stride(0) if g > 1 else max(n, weights.stride(0))
        if ldw < n:
            raise ValueError("rows of weights overlap")
        if self._new_result(out, (shift, limits), "shift and limits", accumulate):
            lim = None
            if limits is not None:
                lim = torch.as_tensor(check_reweigh_limits(limits, s, k), device=dev)
            out = ReweighAccumulator(torch.empty((n, REWEIGH_FIELDS, s, k), dtype=F64, device=dev), torch.empty((n, REWEIGH_JOINT_FIELDS), dtype=F64, device=dev),
                                     self._ensemble_shift(shift, values, g, s, k), lim, scenario_names)
        self._check_tables(f"out must hold contiguous device tables acc [{n}, {REWEIGH_FIELDS}, S, K], joint [{n}, {REWEIGH_JOINT_FIELDS}], shift [S, K] = "
                           f"[{s}, {k}] and limits [S, K, 2]",
                           [(out.acc, (n, REWEIGH_FIELDS, s, k), F64), (out.joint, (n, REWEIGH_JOINT_FIELDS), F64), (out.shift, (s, k), F64)],
                           [(out.limits, (s, k, 2), F64)])
        self._check_mask(mask, g, contiguous=True)
        if verdict is not None and (not isinstance(verdict, torch.Tensor) or verdict.dtype != U8 or tuple(verdict.shape) != (g,) or verdict.device != dev
                                    or not verdict.is_contiguous()):
            raise ValueError("verdict must be a contiguous uint8 [G] device tensor")
        scratch = self._ensemble_scratch("reweigh", int(self.lib.okx_ensemble_reweigh_scratch_bytes(g, s, k, n)))
        self._ensemble_call("okx_ensemble_reweigh", g, s, k, _ptr(values), ld, _ptr(status), stride, _ptr(mask), _ptr(out.shift), _ptr(weights), ldw, n,
                            _ptr(out.limits), _ptr(verdict), 1 if accumulate else 0, _ptr(out.acc), _ptr(out.joint), _ptr(scratch), scratch.numel())
        return out

    # ---- okx_ensemble_basis / okx_ensemble_surface: the normal equations of a polynomial response surface (ensemble_stats.EnsembleSurface) ----

    def _strided_rows(self, t, what: str, letters: str, rows: int | None = None) -> tuple:
        """``(G, columns, ld)`` of ``t``, a float64 ``[G, columns]`` device tensor with unit column stride whose rows may be strided."""
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != F64 or t.device != self.device or (t.shape[1] > 1 and t.stride(1) != 1) \
                or (rows is not None and t.shape[0] != rows):
            raise ValueError(f"{what} must be a float64 {letters} device tensor with unit column stride")
        g, c = t.shape
        ld = t.stride(0) if g > 1 else max(c, t.stride(0))
        if ld < c:
            raise ValueError(f"rows of {what} overlap")
        return g, c, ld

    def basis_factors(self, factors, basis=None, out=None) -> "SurfaceBasisTable":
        """
        ``okx_ensemble_basis``: the basis rows of ``factors [G, P]`` (a float64 device tensor with unit column stride; rows may be strided - the
        sampler's ``latents`` as they lie in HBM) under ``basis`` (``ensemble_stats.surface_terms``; validated on the host and uploaded) as a
        ``SurfaceBasisTable``: ``phi [G, T]`` and ``valid [G]``.  Done ONCE for an ensemble: factors do not change from step to step.  ``out``: the
        ``SurfaceBasisTable`` of an earlier call of the same shape - it carries its own basis (``basis`` may then be None); its ``phi`` may be a
        view with strided rows; with it the call uploads and allocates nothing and is legal inside a stream capture.  The bits of
        ``ensemble_stats.basis_host``.
        """
        g, p, ld = self._strided_rows(factors, "factors", "[G, P]")
        dev = self.device
        if out is None:
            if not isinstance(basis, SurfaceBasis):
                raise ValueError("basis must be the SurfaceBasis of ensemble_stats.surface_terms (or out=, which carries its own)")
            law, terms = check_surface_basis(basis.law, basis.terms)
            rc = self.lib.okx_ensemble_basis_check(law.ctypes.data_as(C.c_void_p), min(law.shape[0], 1 << 20), terms.ctypes.data_as(C.c_void_p), terms.shape[0])
            _lib.check(rc, "okx_ensemble_basis")
            out = SurfaceBasisTable(torch.empty((g, terms.shape[0]), dtype=F64, device=dev), torch.empty(g, dtype=U8, device=dev),
                                    torch.as_tensor(law, device=dev), torch.as_tensor(terms, device=dev), basis)
        elif basis is not None and not basis.same(out.basis):
            raise ValueError("out= carries its own basis")
        t = out.basis.n_terms
        if out.basis.n_factors != p:
            raise ValueError(f"factors must be [G, {out.basis.n_factors}], one column per factor of the basis")
        _, _, ld_phi = self._strided_rows(out.phi, f"out.phi [{g}, {t}]", "[G, T]", rows=g)
        if out.phi.shape[1] != t:
            raise ValueError(f"out.phi must be [{g}, {t}]")
        self._check_tables(f"out must hold contiguous device tables valid [{g}], law [{p}, 3] and terms [{t}, 4]",
                           [(out.valid, (g,), U8), (out.law, (p, 3), F64), (out.terms, (t, 4), I32)])
        self._ensemble_call("okx_ensemble_basis", g, _ptr(factors), ld, p, _ptr(out.law), _ptr(out.terms), t, _ptr(out.phi), ld_phi, _ptr(out.valid))
        return out

    def surface_ensemble(self, values, *, steps_per_geometry: int, basis_table, status=None, mask=None, entries=None, shift=None, out=None,
                         accumulate: bool = False):
        """
        ``okx_ensemble_surface``: the response-surface accumulator (``ensemble_stats.SurfaceAccumulator``, device tensors: ``gram [T, T]``,
        ``cross [T, N]``, ``sumsq [N]``, ``counts [2]`` = used, dropped, ``used [G]`` uint8) of ``entries`` - N distinct indices ``s K + k``, None: all
        ``S K`` - of a column table in HBM over its COMPLETE geometries: every selected entry counts, bit 0 of the mask byte is clear and the
        basis row is valid.  ``values`` and ``status`` as ``reduce_ensemble`` takes them (unit column stride; strided rows and a strided status
        byte are passed on, nothing is copied); ``basis_table``: the ``SurfaceBasisTable`` ``basis_factors`` made of the factors of THESE
        geometries; ``mask [G]`` contiguous uint8 - the sampler's ``flags`` as they lie in HBM.  ``shift [S, K]`` the common shift (None: the
        table's own geometry 0, undefined entries 0 - chunks that are accumulated need ONE shift, pass it or pass ``out=``).  ``out``: the
        accumulator of an earlier call - it carries its own shift, entries and basis - to write (``accumulate=False``) or add into (``True``);
        with it and a table shape seen before, the call uploads and allocates nothing and is legal inside a stream capture (``out.used`` is
        written when it holds a byte per geometry of the call).  ``.finalize()`` copies to the host and solves: coefficients, R^2, variance
        shares.  Bit-identical from run to run; different chunkings agree to rounding.
        """
        g, s, k, ld, stride = self._ensemble_table(values, status, steps_per_geometry)
        dev = self.device
        if not isinstance(basis_table, SurfaceBasisTable):
            raise ValueError("basis_table must be the SurfaceBasisTable of basis_factors")
        t = basis_table.basis.n_terms
        _, _, ld_phi = self._strided_rows(basis_table.phi, f"basis_table.phi [{g}, {t}] (one row per geometry of the table)", "[G, T]", rows=g)
        if basis_table.phi.shape[1] != t:
            raise ValueError(f"basis_table.phi must be [{g}, {t}]")
        self._check_tables(f"basis_table must hold a contiguous device table valid [{g}]", [(basis_table.valid, (g,), U8)])
        if self._new_result(out, (shift, entries), "shift and entries", accumulate):
            host = None if entries is None else np.ascontiguousarray(check_surface_arguments(
                entries.detach().cpu().numpy() if isinstance(entries, torch.Tensor) else entries, s * k, t))
            n = s * k if host is None else host.size
            rc = self.lib.okx_ensemble_surface_check(None if host is None else host.ctypes.data_as(C.c_void_p), min(n, 1 << 30), s * k, t)
            _lib.check(rc, "okx_ensemble_surface")
            shift = self._ensemble_shift(shift, values, g, s, k)
            index = torch.arange(n, dtype=torch.int32, device=dev) if host is None else torch.as_tensor(host, device=dev)
            out = SurfaceAccumulator(torch.empty((t, t), dtype=F64, device=dev), torch.empty((t, n), dtype=F64, device=dev), torch.empty(n, dtype=F64, device=dev),
                                     torch.empty(2, dtype=I64, device=dev), shift, index, torch.empty(g, dtype=U8, device=dev), basis=basis_table.basis,
                                     natural=host is None)  # (all entries in natural order: the call passes no entry list)
        elif not out.basis.same(basis_table.basis):
            raise ValueError("out= was taken with another basis")
        n = _rows(out.entries)
        self._check_tables(f"out must hold contiguous device tables gram [{t}, {t}], cross [{t}, N], sumsq [N], counts [2], entries [N] and shift [S, K] = [{s}, {k}]",
                           [(out.gram, (t, t), F64), (out.cross, (t, n), F64), (out.sumsq, (n,), F64), (out.counts, (2,), I64), (out.shift, (s, k), F64),
                            (out.entries, (n,), I32)])
        self._check_mask(mask, g, contiguous=True)
        used = out.used  # (written when it holds a byte per geometry of the call)
        if used is not None and (used.dtype != U8 or used.shape[0] < g or not used.is_contiguous() or used.device != dev):
            used = None
        scratch = self._ensemble_scratch("surface", int(self.lib.okx_ensemble_surface_scratch_bytes(g, s, k, t, n)))
        index = None if out.natural and n == s * k else _ptr(out.entries)
        self._ensemble_call("okx_ensemble_surface", g, s, k, _ptr(values), ld, _ptr(status), stride, _ptr(mask), _ptr(basis_table.phi), ld_phi,
                            _ptr(basis_table.valid), t, index, n, _ptr(out.shift), 1 if accumulate else 0, _ptr(out.gram), _ptr(out.cross), _ptr(out.sumsq),
                            _ptr(out.counts), _ptr(used), _ptr(scratch), scratch.numel())
        return out

    def predict_surface(self, surface, factors) -> torch.Tensor:
        """
        The fitted entries ``float64 [G, N]`` of ``surface`` (``ensemble_stats.EnsembleSurface``, host) at ``factors [G, P]`` on the device, without
        a solve: the basis pass, then ``shift + phi @ coefficients`` (``torch.matmul``); NaN where a factor is not finite.  Host form:
        ``EnsembleSurface.predict``.  ``predict_ensemble`` gives the same table from one launch, without the basis table in memory and with
        defined bits.
        """
        table = self.basis_factors(factors, surface.basis)
        out = torch.as_tensor(surface.shift, device=self.device)[None, :] + torch.matmul(table.phi, torch.as_tensor(surface.coefficients, device=self.device))
        return torch.where(table.valid[:, None] != 0, out, torch.full_like(out, float("nan")))

    # ---- okx_ensemble_predict: the fitted surface as a column table (ensemble_stats.predict_host), and its leave-one-out error ----

    def upload_surface(self, surface) -> "SurfaceModel":
        """
        The tables of ``surface`` (``ensemble_stats.EnsembleSurface``, host) on the device as a ``SurfaceModel``: validated on the host
        (``okx_ensemble_basis_check``, ``okx_ensemble_predict_check``) and uploaded ONCE, so that ``predict_ensemble`` uploads nothing.
        """
        basis = surface.basis
        if not isinstance(basis, SurfaceBasis):
            raise ValueError("surface must be an EnsembleSurface (SurfaceAccumulator.finalize)")
        law, terms = check_surface_basis(basis.law, basis.terms)
        rc = self.lib.okx_ensemble_basis_check(law.ctypes.data_as(C.c_void_p), min(law.shape[0], 1 << 20), terms.ctypes.data_as(C.c_void_p), terms.shape[0])
        _lib.check(rc, "okx_ensemble_basis")
        c, shift, _ = check_predict_arguments(basis, surface.coefficients, surface.shift)
        entries = np.ascontiguousarray(np.asarray(surface.entries).reshape(-1).astype(np.int32))
        if entries.size != c.shape[1]:
            raise ValueError(f"surface.entries must be [N] = [{c.shape[1]}]")
        rc = self.lib.okx_ensemble_predict_check(None, min(c.shape[1], 1 << 30), 0, terms.shape[0], min(law.shape[0], 1 << 20))
        _lib.check(rc, "okx_ensemble_predict")
        dev = self.device
        whitener = getattr(surface, "whitener", None)
        return SurfaceModel(torch.as_tensor(law, device=dev), torch.as_tensor(terms, device=dev), _as_f64(c, dev), _as_f64(shift, dev),
                            torch.as_tensor(entries, device=dev), None if whitener is None else _as_f64(whitener, dev), basis, entries)

    def predict_ensemble(self, model, factors, *, mask=None, values=None, status=None, steps_per_geometry=None, coefficients=None, out=None,
                         valid=None) -> tuple:
        """
        ``okx_ensemble_predict``: ``(out [G, N], valid [G])``, the surface of ``model`` (``upload_surface``) at ``factors [G, P]`` (a float64
        device tensor with unit column stride; rows may be strided - the sampler's ``latents`` as they lie in HBM) as a column table that
        every ensemble pass reads with ``steps_per_geometry=1`` - one launch, the basis table never lies in memory.  ``mask [G]`` contiguous
        uint8 (the sampler's ``flags``): bit 0 set drops the row.  A dropped row, or one with a factor that is not finite, is NaN in every
        column and has ``valid = 0``.  With ``values`` (and ``status``, ``steps_per_geometry``, as ``reduce_ensemble`` takes them) the call
        runs RESIDUAL mode: ``value - prediction`` of the model's entries, NaN where the entry does not count.  ``coefficients``: another
        ``[T, N']`` device matrix (unit column stride) in the place of the model's, with a zero shift - how the whitener goes through.
        ``out`` (``[G, N]``, rows may be strided: columns of a wider table) and ``valid`` (``[G]`` uint8): with both the call allocates and
        uploads nothing and is legal inside a stream capture.  ROW-PURE: a geometry's row has the same bits in every chunking, on every
        device and in every call (``include/okx.h``); ``ensemble_stats.predict_host`` within the bound stated there.
        """
        if not isinstance(model, SurfaceModel):
            raise ValueError("model must be the SurfaceModel of upload_surface")
        g, p, ld = self._strided_rows(factors, "factors", "[G, P]")
        t = model.basis.n_terms
        if model.basis.n_factors != p:
            raise ValueError(f"factors must be [G, {model.basis.n_factors}], one column per factor of the basis")
        self._check_tables(f"model must hold contiguous device tables law [{p}, 3] and terms [{t}, 4]", [(model.law, (p, 3), F64), (model.terms, (t, 4), I32)])
        shift = None
        if coefficients is None:
            coefficients, shift = model.coefficients, model.shift
        _, n, ld_c = self._strided_rows(coefficients, f"coefficients [{t}, N]", "[T, N]", rows=t)
        self._check_tables(f"model must hold a contiguous device table shift [{n}]", [], [(shift, (n,), F64)])
        self._check_mask(mask, g, contiguous=True)
        mode, s, k, ld_v, stride, index = PREDICT_VALUE, 0, 0, 0, 0, None
        if values is not None:
            if steps_per_geometry is None:
                raise ValueError("steps_per_geometry is needed with values=")
            gv, s, k, ld_v, stride = self._ensemble_table(values, status, steps_per_geometry)
            if gv != g:
                raise ValueError(f"values must hold {g} geometries, one per factor row")
            host = model.entries_host
            if host.size != n:
                raise ValueError(f"okx_ensemble_predict: {host.size} entries of the table for {n} columns of the coefficients")
            self._check_tables(f"model must hold a contiguous device table entries [{n}]", [(model.entries, (n,), I32)])
            rc = self.lib.okx_ensemble_predict_check(host.ctypes.data_as(C.c_void_p), min(host.size, 1 << 30), s * k, t, p)
            _lib.check(rc, "okx_ensemble_predict")
            mode, index = PREDICT_RESIDUAL, model.entries
        elif status is not None:
            raise ValueError("status= goes with values=")
        dev = self.device
        if out is None:
            out = torch.empty((g, n), dtype=F64, device=dev)
        _, _, ld_out = self._strided_rows(out, f"out [{g}, {n}]", "[G, N]", rows=g)
        if out.shape[1] != n:
            raise ValueError(f"out must be [{g}, {n}]")
        if valid is None:
            valid = torch.empty(g, dtype=U8, device=dev)
        self._check_tables(f"valid must be a contiguous uint8 [{g}] device tensor", [(valid, (g,), U8)])
        self._ensemble_call("okx_ensemble_predict", g, mode, _ptr(factors), ld, p, _ptr(model.law), _ptr(model.terms), t, _ptr(coefficients), ld_c, n,
                            _ptr(shift), _ptr(mask), s, k, _ptr(values), ld_v, _ptr(status), stride, _ptr(index), _ptr(out), ld_out, _ptr(valid))
        return out, valid

    def validate_surface(self, model, surface, factors, values, *, steps_per_geometry: int, status=None, mask=None, used=None, chunk: int = 16384):
        """
        The leave-one-out error of a fit over the geometries it was fitted on (``ensemble_stats.SurfaceValidation``; the definition is
        ``ensemble_stats.surface_validate_host``): one RESIDUAL call of ``predict_ensemble`` for ``e``, one VALUE call with the whitener per
        ``chunk`` geometries for the leverage ``h = |phi_g whitener|^2`` (``[chunk, T]`` bounds the memory), then ``e_loo = e / (1 - h)`` and
        its sums with torch's elementwise operations on the device.  ``used [G]``: the used bytes of the fit (``SurfaceAccumulator.used``);
        None: the rows whose residuals are all defined - the complete cases.  NOT bit-defined: the row norms and the sums are torch's.
        """
        if model.whitener is None or getattr(surface, "total_ss", None) is None:
            raise ValueError("the surface carries no whitener (SurfaceAccumulator.finalize fills it)")
        e, _ = self.predict_ensemble(model, factors, mask=mask, values=values, status=status, steps_per_geometry=steps_per_geometry)
        g = e.shape[0]
        keep = torch.isfinite(e).all(dim=1) if used is None else torch.as_tensor(used, device=self.device).reshape(-1) != 0
        if keep.shape[0] != g:
            raise ValueError(f"used must be [G] = [{g}]")
        h = torch.empty(g, dtype=F64, device=self.device)
        step = max(1, int(chunk))
        for a in range(0, g, step):
            z, _ = self.predict_ensemble(model, factors[a:a + step], coefficients=model.whitener)
            h[a:a + step] = (z * z).sum(dim=1)
        count = int(keep.sum().item())
        if count == 0:
            return validation_from_terms(np.zeros((0, e.shape[1])), np.zeros(0), np.zeros(0), np.asarray(surface.total_ss, dtype=np.float64))
        loo = torch.where(keep[:, None], e / (1.0 - h)[:, None], torch.zeros((), dtype=F64, device=self.device))
        ss = (loo * loo).sum(dim=0).cpu().numpy()
        worst, at = loo.abs().max(dim=0)
        total_ss = np.asarray(surface.total_ss, dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            q2 = np.where(total_ss > 0.0, 1.0 - ss / total_ss, np.nan)
        zero, low = torch.zeros((), dtype=F64, device=self.device), torch.full((), float("-inf"), dtype=F64, device=self.device)
        return SurfaceValidation(np.sqrt(ss / count), q2, worst.cpu().numpy(), at.cpu().numpy().astype(np.int64), float(torch.where(keep, h, low).max().item()),
                                 float(torch.where(keep, h, zero).sum().item()) / count, count)
