"""
What the on-device curve characteristics cost (okx_ensemble_curves, DeviceProgram.curves_ensemble) on BASELINE config 5 - 4096
perturbed geometries x 256 bump steps, bench.py's four metric columns - on ONE GPU, device events, 20 repetitions after warm-up,
all in one run and alternated block by block so that a drift hits every pass alike:

  (a) the curves pass for D = 1 and D = 3, with the shared abscissa (the relative bump targets) and with a column of the table
      as the abscissa;
  (b) on the same table: okx_ensemble_screen and okx_ensemble_reduce - passes that read the same bytes once;
  (c) what the user must otherwise do: metric_local.cpu() (timed alone), then ensemble_stats.curves_host (timed on a slice of
      the geometries and scaled - it is a Python loop over (geometry, column)).

The pass reads the table once from HBM and once more from L2 and writes 100 bytes per (geometry, column).  The expectation -
recorded, not a gate - is (a) within 3 x the screen pass of (b); the ratio is in the output either way.

  python tools/ensemble_curves_rate.py --out profiles/r15/ensemble_curves_rate.json

``--rehearse N``: N ranks on cuda:0 over gloo (fresh child processes) run ShardedEnsemble(reduce=True, factors="hardpoints",
curves=...) and write their curve statistics and local feature tables to ``<out>/rank<r>.pt`` - the rehearsal
tests/test_gpu_ensemble_curves.py compares.
"""

from __future__ import annotations

import os
import statistics
import sys
import time

import ensemble_rate_common as common
from ensemble_rate_common import alternated, rank, spread
from ensemble_reduce_rate import HBM_PEAK, build

STAT_FIELDS = ("count", "rejected", "mean", "variance", "std", "min", "max", "argmin", "argmax", "sensitivity", "intercept", "r2")


def curve_arguments(rel, degree: int = 2, column: bool = False) -> dict:
    """The ensemble's curves= arguments: the relative bump targets as the shared abscissa (their half range as the scale, a
    window of 0.8 of it), or column 0 of the chosen columns (camber) against which the others are fitted."""
    import numpy as np

    x = np.asarray(rel, dtype=np.float64)[:, -1]
    half = float(max(np.max(np.abs(x)), 1.0))
    if column:
        return dict(abscissa=0, origin=0.0, scale=1.0, degree=degree, window=None)
    return dict(abscissa=x, origin=0.0, scale=half, degree=degree, window=(-0.8 * half, 0.8 * half))


def rank_main(args) -> None:
    import dataclasses

    import torch

    from open_kinematics_amd.dist import ShardedEnsemble

    with rank(args) as device:
        dp, table, rel, columns = build(args.geometries, args.steps_per_geometry, device)
        pipe = ShardedEnsemble(dp, table, rel, args.steps_per_geometry, chunks=args.chunks or None, metric_columns=columns, reduce=True,
                               factors="hardpoints" if args.geometries > 2 else None, curves=curve_arguments(rel), chain_len=1, predictor=False)
        acc = pipe.step()
        torch.cuda.synchronize()
        stats, local = pipe.curve_stats(), pipe.curves_local()
        torch.save({"stats": {f.name: getattr(stats, f.name) for f in dataclasses.fields(stats)}, "features": local.features.cpu(), "count": local.count.cpu(),
                    "acc": acc.acc.cpu(), "sent": pipe.exchange_bytes_per_rank, "curves_sent": pipe.curves_exchange_bytes_per_rank,
                    "range": pipe.geometry_range, "n_factors": pipe.n_factors},
                   os.path.join(args.out, f"rank{args.rank}.pt"))


def rehearse(args) -> int:
    return common.rehearse(args, __file__, 40500, ["--geometries", args.geometries, "--steps-per-geometry", args.steps_per_geometry,
                                                        "--chunks", args.chunks])


def measure(args) -> dict:
    import numpy as np
    import torch

    from open_kinematics_amd.dist import ShardedEnsemble
    from open_kinematics_amd.ensemble_stats import EnsembleAccumulator, curves_host

    device = torch.device("cuda:0")
    g, s = args.geometries, args.steps_per_geometry
    dp, table, rel, columns = build(g, s, device)
    k = len(columns)
    reduced = ShardedEnsemble(dp, table, rel, s, metric_columns=columns, reduce=True, chain_len=1, predictor=False)
    for _ in range(max(1, args.warmup)):
        reduced.step()
    torch.cuda.synchronize()
    values, status = reduced.metric_local, reduced.info_local[:, 32]
    reps = args.reps

    passes = {}
    outs = {}
    for degree in (1, 3):
        for kind in ("shared", "column"):
            kw = curve_arguments(rel, degree, kind == "column")
            out = dp.curves_ensemble(values, steps_per_geometry=s, status=status, **kw)
            outs[degree, kind] = (out, kw)
            passes[f"curves_d{degree}_{kind}"] = lambda out=out: dp.curves_ensemble(values, steps_per_geometry=s, status=status, out=out)
    limits = np.tile(np.array([-1e6, 1e6]), (s, k, 1))
    scr = dp.screen_ensemble(values, steps_per_geometry=s, status=status, limits=limits)
    passes["screen"] = lambda: dp.screen_ensemble(values, steps_per_geometry=s, status=status, out=scr)
    acc = EnsembleAccumulator(torch.empty_like(reduced.local_accumulator.acc), reduced.local_accumulator.shift, None)
    passes["reduce"] = lambda: dp.reduce_ensemble(values, steps_per_geometry=s, status=status, out=acc)
    runs = alternated(passes, reps)
    med = {name: statistics.median(r) for name, r in runs.items()}

    # (c) the host route: the copy alone, then curves_host on a slice of the geometries
    copy_ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = values.cpu()
        copy_ms.append((time.perf_counter() - t0) * 1e3)
    part = min(g, 64)
    host_v, host_st = host.numpy().reshape(g, s, k)[:part], status.cpu().numpy().reshape(g, s)[:part]
    out, kw = outs[3, "shared"]
    t0 = time.perf_counter()
    want = curves_host(host_v, host_st, **kw)
    host_ms = (time.perf_counter() - t0) * 1e3 * g / part
    got = out.finalize()
    exact = bool(np.array_equal(got.count[:part], want.count) and
                 np.array_equal(got.features[:part, :, 6:].view(np.uint64), want.features[..., 6:].view(np.uint64)))
    with np.errstate(invalid="ignore"):
        fit_gap = float(np.nanmax(np.abs(got.features[:part, :, :4] - want.features[..., :4]) * kw["scale"] ** np.arange(4)))
    table_bytes = 8 * g * s * k + g * s
    written = g * k * 100
    curves = {name: {"median": med[name], "interquartile": spread(runs[name]), "over_screen": med[name] / med["screen"],
                     "bytes_per_s_of_the_table_once": table_bytes / (med[name] * 1e-6), "runs": runs[name]} for name in passes if name.startswith("curves")}
    worst = max(c["over_screen"] for c in curves.values())
    return {
        "workload": f"C5: {g} geometries x {s} steps, {k} metric columns, one GPU",
        "a_curves_pass_us": curves,
        "b_same_table_us": {name: {"median": med[name], "interquartile": spread(runs[name]), "runs": runs[name]} for name in ("screen", "reduce")},
        "table_bytes": table_bytes, "bytes_written": written, "hbm_floor_us": (table_bytes + written) / HBM_PEAK * 1e6,
        "expectation_within_3x_of_the_screen_pass": {"worst_ratio": worst, "holds": bool(worst <= 3.0)},
        "c_host_path_ms": {"copy_alone_median": statistics.median(copy_ms), "copy_runs": copy_ms, "curves_host_scaled_from": part,
                           "curves_host": host_ms},
        "device_equals_curves_host": {"count_and_fields_6_to_11_exactly": exact, "largest_coefficient_gap_in_u_units": fit_gap},
        "fitted_fraction": float(np.mean(np.isfinite(got.features[..., 0]))),
    }


def summary(r: dict) -> str:
    lines = [r["workload"]]
    for name, c in r["a_curves_pass_us"].items():
        lines.append(f"(a) {name:<22} {c['median']:8.1f} us  (interquartile {c['interquartile']:.1f})   / screen = {c['over_screen']:.2f}   "
                     f"{c['bytes_per_s_of_the_table_once'] / 1e12:.2f} TB/s of the table read once")
    for name, c in r["b_same_table_us"].items():
        lines.append(f"(b) {name:<22} {c['median']:8.1f} us  (interquartile {c['interquartile']:.1f})")
    e, c, d = r["expectation_within_3x_of_the_screen_pass"], r["c_host_path_ms"], r["device_equals_curves_host"]
    lines.append(f"    expectation, curves within 3 x the screen pass: worst ratio {e['worst_ratio']:.2f} - " + ("holds" if e["holds"] else "MISSED"))
    lines.append(f"    the table and the features at the HBM peak: {r['hbm_floor_us']:.1f} us")
    lines.append(f"(c) copy alone {c['copy_alone_median'] * 1e3:.1f} us, curves_host {c['curves_host']:.0f} ms (scaled from {c['curves_host_scaled_from']} geometries)")
    lines.append(f"    device == curves_host: count and fields 6 .. 11 exactly {d['count_and_fields_6_to_11_exactly']}, largest coefficient gap "
                 f"{d['largest_coefficient_gap_in_u_units']:.2e} (u units); fitted {r['fitted_fraction']:.4f} of the rows")
    return "\n".join(lines) + "\n"


def main() -> int:
    ap = common.parser(geometries=4096, steps_per_geometry=256, warmup=3, reps=20, chunks=0)
    return common.run(ap.parse_args(), measure, summary, rank_main, rehearse)


if __name__ == "__main__":
    sys.exit(main())
