"""
The VIRTUAL ensemble: millions of geometries drawn on the device and run through a fitted response surface instead of the solver, then
counted by the passes that read any column table.  4096 solved geometries resolve a yield of 99 %; 50 ppm or a 0.9999 quantile need the
surrogate.

Per chunk of geometries ``[a, b)`` of the plan: ``sample_ensemble(plan, a, b, latents=True, out=...)`` draws, ``predict_ensemble(model,
latents, mask=flags, out=table)`` evaluates, and the consumers read ``table [b - a, N]`` with ``steps_per_geometry=1``:
``reduce_ensemble(accumulate=)`` for the moments and extremes, ``screen_ensemble(geometry_offset=)`` for the joint verdicts (merged on the
host) and the select pass's own rounds for the quantiles and per-entry limit counts.  Every count round of the select draws and predicts the
chunks AGAIN instead of keeping them.  That is only correct because the sampler is counter-based - a geometry's draw is a function of
(seed, index) - and the prediction is row-pure - a geometry's row is a function of its factors and the model alone: the chunk of round 7
is the chunk of round 0, bit for bit.  Device memory is ONE chunk, whatever ``hi - lo`` is.

One process, one device; ``lo`` / ``hi`` let a caller split the range.
"""

from __future__ import annotations

from dataclasses import dataclass

import torch

from .ensemble_device import EnsembleSample
from .ensemble_stats import EnsembleQuantiles, EnsembleScreen, EnsembleStats


@dataclass
class VirtualEnsemble:
    """
    What ``virtual_ensemble`` returns (host): ``stats`` (``EnsembleStats`` of the ``[1, N]`` entries; argmin / argmax are indices of the plan),
    ``quantiles`` (``EnsembleQuantiles`` with the per-entry limit counts; None without ``probs``), ``screen`` (``EnsembleScreen``: joint yield,
    blame counts and - with ``verdicts`` - the per-geometry tables; None unless asked for), and the counts: ``drawn`` geometries, ``dropped`` of
    them by the sampler's guards (flag bit 0), ``invalid`` rows of the table (dropped ones included: NaN rows, which no pass counts).
    """

    stats: EnsembleStats
    quantiles: EnsembleQuantiles | None
    screen: EnsembleScreen | None
    drawn: int
    dropped: int
    invalid: int


def virtual_ensemble(dp, model, plan, lo: int = 0, hi: int | None = None, *, chunk: int = 65536, probs=None, limits=None, scale=None,
                     screen: bool = False, verdicts: bool = True) -> VirtualEnsemble:
    """
    Geometries ``[lo, hi)`` (``hi`` None: ``plan.n_total``) of ``plan`` through ``model`` (``DeviceProgram.upload_surface``; its factors are the
    plan's latents) in chunks of ``chunk``.  ``probs [Q]``: the quantiles wanted (``select`` rounds; with ``limits [N, 2]`` or ``[2]`` also the
    per-entry counts below / above).  ``screen=True`` (needs ``limits``; ``scale`` as ``screen_ensemble`` takes it): the joint verdict;
    ``verdicts=False`` keeps its tally and blame counts only, not the per-geometry tables.  Integer results - counts, order statistics,
    verdicts - are the same bits for every ``chunk``; the floating sums of the moments follow ``reduce_ensemble``'s chunk rule (rounding).
    """
    lo = int(lo)
    hi = int(plan.n_total) if hi is None else int(hi)
    chunk = int(chunk)
    if lo < 0 or hi < lo or chunk < 1:
        raise ValueError(f"bad range [{lo}, {hi}) or chunk {chunk}")
    if model.basis.n_factors != plan.n_latents:
        raise ValueError(f"the model has {model.basis.n_factors} factors, the plan {plan.n_latents} latents")
    if screen and limits is None:
        raise ValueError("screen=True needs limits")
    n = int(model.coefficients.shape[1])
    dev = dp.device
    rows = max(1, min(chunk, hi - lo))
    sample = EnsembleSample(torch.empty((rows, plan.n_points, 3), dtype=torch.float64, device=dev),
                            torch.empty((rows, plan.n_latents), dtype=torch.float64, device=dev), None, torch.empty(rows, dtype=torch.uint8, device=dev))
    table = torch.empty((rows, n), dtype=torch.float64, device=dev)
    valid = torch.empty(rows, dtype=torch.uint8, device=dev)
    edges = list(range(lo, hi, chunk)) + [hi]

    def chunks():
        """``(a, table rows, flags, valid)`` of every chunk, drawn and predicted into the one set of buffers."""
        for a, b in zip(edges[:-1], edges[1:]):
            m = b - a
            part = sample if m == rows else EnsembleSample(sample.hardpoints[:m], sample.latents[:m], None, sample.flags[:m])
            dp.sample_ensemble(plan, a, b, latents=True, out=part)
            dp.predict_ensemble(model, part.latents, mask=part.flags, out=table[:m], valid=valid[:m])
            yield a, table[:m], part.flags, valid[:m]

    shift = model.shift.reshape(1, n)
    acc, screened, dropped, invalid = None, None, 0, 0
    run = None if probs is None else dp.select_prepare(1, n, probs, limits, rounds=True)
    held = dp.screen_prepare(1, n, limits, scale, rows) if screen else None
    if run is not None:
        dp.select_begin(run)
    bad = torch.zeros(2, dtype=torch.int64, device=dev)
    for a, part, flags, ok in chunks():  # the first sweep: moments, verdicts, the counts - and round 0 of the select
        acc = dp.reduce_ensemble(part, steps_per_geometry=1, shift=shift if acc is None else None, geometry_offset=a, out=acc, accumulate=acc is not None)
        bad[0] += (flags & 1).sum()
        bad[1] += (ok == 0).sum()
        if run is not None:
            dp.select_count(run, 0, part, steps_per_geometry=1)
        if held is not None:
            dp.screen_ensemble(part, steps_per_geometry=1, geometry_offset=a, out=held, first_row=0)
            piece = held.finalize()
            if not verdicts:
                piece = EnsembleScreen(piece.flags[:0], None, None, piece.tally, piece.blame, piece.passed[:0])
            screened = piece if screened is None else screened.merge(piece)
    if acc is None:  # no geometry at all
        acc = dp.reduce_ensemble(table[:0], steps_per_geometry=1, shift=shift)
    if run is not None:
        dp.select_descend(run, 0)
        for rnd in range(1, dp.select_rounds):
            for _, part, _, _ in chunks():
                dp.select_count(run, rnd, part, steps_per_geometry=1)
            dp.select_descend(run, rnd)
        dp.select_finish(run)
    dropped, invalid = (int(x) for x in bad.tolist())
    return VirtualEnsemble(acc.finalize(), None if run is None else run.finalize(), screened, hi - lo, dropped, invalid)
