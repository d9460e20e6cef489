"""
What the main-effects passes cost (okx_ensemble_bin, okx_ensemble_effects) on BASELINE config 5's shape - geometries of the perturbed
double wishbone drawn by the sampler (LHS, 30 latents) x 256 bump steps, bench.py's four metric columns - with 16 bins, for the
first 10 and for all 30 latents as factors, at 4096 geometries (C5, a 33.6 MB table) and at 131 072 (a 1.07 GB table), on ONE GPU,
device events, 20 repetitions after warm-up, alternated block by block so that a drift hits every pass alike:

  (a) the bin pass (once per ensemble: factors do not change from step to step);
  (b) the effects pass over the evaluated table, beside okx_ensemble_reduce (no factors) over the same table; the pass walks the
      table once per factor, so its effective traffic is F table reads - reported with the rate that makes;
  (c) what the user must otherwise do: the table's .cpu() (timed alone), then ensemble_stats.effects_host (NumPy).

Nobody had measured this pass; no target is fixed.  The device accumulator is compared with effects_host's: COUNT equal, the sums
within 2 (n + 1) u sum |term| of the host's own terms, n the geometries of the cell's bin.

  python tools/ensemble_effects_rate.py --out profiles/r23/ensemble_effects_rate.json
"""

from __future__ import annotations

import statistics
import sys
import time

import ensemble_rate_common as common
from ensemble_rate_common import timed

U = 2.0 ** -53


def build(n_geom: int, steps: int, device, *, n_points=None, stratify: int = 1):
    """The C5 plan (``workloads.ensemble_plan``; ``n_points``: over the first authored points only), its program on ``device`` with the
    evaluation enabled, the relative targets and bench.py's four metric columns."""
    from open_kinematics_amd.batch import DeviceProgram
    from open_kinematics_amd.ensemble_sample import hardpoint_plan
    from open_kinematics_amd.input import load_geometry
    from open_kinematics_amd.metrics import corner_roles
    from open_kinematics_amd.workloads import ensemble_plan, geometry_path

    program, plan, rel = ensemble_plan(n_geom, 1.0, 3, n_steps=steps, stratify=stratify)
    if n_points is not None:
        points = sorted({int(c) // 3 for c in plan.coords})[:n_points]
        plan = hardpoint_plan(program, points, sigma=1.0, stratify=stratify, n_total=n_geom, seed=3, guards=plan.guards, max_attempts=plan.max_attempts)
    dp = DeviceProgram(program, device)
    dp.enable_evaluation(corner_roles(load_geometry(geometry_path("geometry.yaml")), program))
    bump = program.n_targets - 1
    columns = [("camber", None), ("camber", bump), ("roadwheel_angle", bump), (21, bump)]
    return dp, plan, rel, columns


def host_bound(values, status, mask, bins, n_bins, shift):
    """``[F, B, 3, S, K]``: 2 (n + 1) u sum |term| of the host's own terms, n the geometries of the cell's bin (COUNT: 0, it is exact).  The
    sums of |term| are taken as one-hot products (their own rounding is far below the factor 2)."""
    import numpy as np

    from open_kinematics_amd.ensemble_stats import EFFECTS_FIELDS, EFFECTS_SUM, EFFECTS_SUMSQ, effects_terms

    _, d, _ = effects_terms(values, status, mask, shift)
    shape = d.shape[1:]
    d = np.abs(d).reshape(d.shape[0], -1)
    sq = d * d
    out = np.zeros((bins.shape[1], n_bins, EFFECTS_FIELDS) + shape)
    for j in range(bins.shape[1]):
        hot = (bins[:, j][None, :] == np.arange(n_bins, dtype=np.uint8)[:, None]).astype(np.float64)  # [B, G]
        scale = (2.0 * (hot.sum(axis=1) + 1.0) * U)[:, None]
        out[j, :, EFFECTS_SUM] = (scale * (hot @ d) * (1.0 + 1e-9)).reshape((n_bins,) + shape)
        out[j, :, EFFECTS_SUMSQ] = (scale * (hot @ sq) * (1.0 + 1e-9)).reshape((n_bins,) + shape)
    return out


def measure_one(args, n_geom: int) -> list:
    import numpy as np
    import torch

    from open_kinematics_amd.dist import ShardedEnsemble
    from open_kinematics_amd.ensemble_stats import EFFECTS_COUNT, bin_factors_host, effects_edges, effects_host

    device = torch.device("cuda:0")
    s, b, reps = args.steps_per_geometry, args.bins, args.reps
    dp, plan, rel, columns = build(n_geom, s, device)
    k = len(columns)
    pipe = ShardedEnsemble(dp, plan, rel, s, metric_columns=columns, reduce=True, factors="sampled", effects=b, chain_len=1, predictor=False)
    t0 = time.perf_counter()
    pipe.step()
    torch.cuda.synchronize()
    first_step_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    pipe.step()
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t0) * 1e3
    table, status, flags, latents = pipe.metric_local, pipe.info_local[:, 32], pipe.sampled_flags, pipe.my_factors
    shift = pipe.local_accumulator.shift
    table_bytes = 8 * n_geom * s * k
    all_edges = effects_edges(plan, b)
    result = pipe.effects()
    mid = s // 2
    strongest = np.argsort(-np.nan_to_num(result.first[:, mid, 0]))[:3]
    chain = {"step_ms": {"first": first_step_ms, "second": step_ms}, "geometries_counted_min_max": [int(result.total_count.min()), int(result.total_count.max())],
             "camber_at_mid_sweep_strongest": [{"factor": result.factor_names[j], "first": float(result.first[j, mid, 0]),
                                                "first_corrected": float(result.first_corrected[j, mid, 0])} for j in strongest]}
    # the host route's copy, once per table
    copy_ms = []
    for _ in range(max(1, reps // 4)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = table.cpu()
        copy_ms.append((time.perf_counter() - t0) * 1e3)
    values = host.numpy().reshape(n_geom, s, k)
    st, fl, sh, lat = status.cpu().numpy().reshape(n_geom, s), flags.cpu().numpy(), shift.cpu().numpy(), latents.cpu().numpy()
    racc = dp.reduce_ensemble(table, steps_per_geometry=s, status=status, shift=shift)
    out = []
    for f in (int(x) for x in args.factors.split(",")):
        factors, edges = latents[:, :f], all_edges[:f]  # (a strided view: ldf stays 30)
        bins = dp.bin_factors(factors, edges)
        acc = dp.effects_ensemble(table, steps_per_geometry=s, bins=bins, status=status, mask=flags, shift=shift)
        runs = timed(reps=reps, passes={"bin": lambda: dp.bin_factors(factors, out=bins),
                                        "effects": lambda: dp.effects_ensemble(table, steps_per_geometry=s, bins=bins, status=status, mask=flags, out=acc),
                                        "reduce": lambda: dp.reduce_ensemble(table, steps_per_geometry=s, status=status, out=racc)})
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_bins = bin_factors_host(lat[:, :f], edges)
        want = effects_host(values, st, fl, host_bins, b, sh, edges)
        host_ms = (time.perf_counter() - t0) * 1e3
        got = acc.numpy().acc
        bound = host_bound(values, st, fl, host_bins, b, sh)
        out.append({
            "workload": f"C5 sampled (LHS): {n_geom} geometries x {s} steps, {k} metric columns, {f} factors x {b} bins, one GPU",
            "a_bin_us": runs["bin"],
            "b_effects_us": runs["effects"],
            "b_reduce_us": runs["reduce"],
            "effects_over_reduce": runs["effects"]["median"] / runs["reduce"]["median"],
            "table_bytes": table_bytes,
            "table_reads": f,
            "effective_bytes_over_table_bytes": float(f) + (4.0 * f * n_geom) / table_bytes,  # F walks of the table, and the lists
            "effective_bytes_per_s": f * table_bytes / (runs["effects"]["median"] * 1e-6),
            "wavefronts": ((s * k + 63) // 64) * f * b,
            "c_host_path_ms": {"copy_alone_median": statistics.median(copy_ms), "copy_runs": copy_ms, "bin_factors_host_and_effects_host": host_ms},
            "bins_equal_the_host": bool(np.array_equal(bins.bins.cpu().numpy(), host_bins)),
            "count_equals_effects_host": bool(np.array_equal(got[:, :, EFFECTS_COUNT], want.acc[:, :, EFFECTS_COUNT])),
            "device_within_bound_of_effects_host": bool(np.all(np.abs(got - want.acc) <= bound)),
            "largest_difference_over_bound": float(np.max(np.abs(got - want.acc) / np.where(bound > 0, bound, 1.0))),
            "chain": chain if f == latents.shape[1] else None,
        })
    return out


def measure(args) -> list:
    results = []
    for n_geom in (int(x) for x in args.geometries.split(",")):
        results += measure_one(args, n_geom)
    return results


def summary(results: list) -> str:
    lines = []
    for r in results:
        a, b, rd, h = r["a_bin_us"], r["b_effects_us"], r["b_reduce_us"], r["c_host_path_ms"]
        lines.append(r["workload"])
        lines.append(f"(a) bin     {a['median']:10.1f} us (interquartile {a['interquartile']:.1f})")
        lines.append(f"(b) effects {b['median']:10.1f} us (interquartile {b['interquartile']:.1f})   reduce, same table {rd['median']:9.1f} us   ratio "
                     f"{r['effects_over_reduce']:.2f}   {r['wavefronts']} wavefronts, {r['table_bytes'] / 1e6:.0f} MB read {r['table_reads']} times "
                     f"({r['effective_bytes_over_table_bytes']:.2f} with the lists): {r['effective_bytes_per_s'] / 1e12:.2f} TB/s effective")
        lines.append(f"(c) host route: copy alone {h['copy_alone_median']:.1f} ms, then bin_factors_host + effects_host {h['bin_factors_host_and_effects_host']:.0f} ms;   "
                     f"bins equal: {r['bins_equal_the_host']}, COUNT equal: {r['count_equals_effects_host']}, sums within 2 (n + 1) u sum |term|: "
                     f"{r['device_within_bound_of_effects_host']} (largest {r['largest_difference_over_bound']:.3f} of the bound)")
        if r["chain"]:
            c = r["chain"]
            top = ", ".join(f"{t['factor']} {t['first']:.3f} ({t['first_corrected']:.3f} corrected)" for t in c["camber_at_mid_sweep_strongest"])
            lines.append(f"    chain step (rebind, evaluated solve, reduce, effects): {c['step_ms']['second']:.1f} ms; camber at mid sweep, strongest factors: {top}")
    return "\n".join(lines) + "\n"


def main() -> int:
    ap = common.parser(rehearsal=False, steps_per_geometry=256, bins=16, reps=20)
    ap.add_argument("--geometries", default="4096,131072", help="the ensemble sizes to measure")
    ap.add_argument("--factors", default="10,30", help="how many of the plan's 30 latents are the factors")
    return common.run(ap.parse_args(), measure, summary)


if __name__ == "__main__":
    sys.exit(main())
