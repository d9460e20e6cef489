"""
What the tolerance what-if passes cost (okx_ensemble_tilt_weights, okx_ensemble_reweigh) on BASELINE config 5's shape - geometries of
the perturbed double wishbone drawn by the sampler (LHS, 30 latents) x 256 bump steps, bench.py's four metric columns - for 8 and for 64
scenarios that tighten three latents, at 4096 geometries (C5, a 33.6 MB table) and at 131 072 (a 1.07 GB table), on ONE GPU, device
events, 20 repetitions after warm-up, alternated block by block so that a drift hits every pass alike:

  (a) the weights pass (once per ensemble: latents do not change from step to step);
  (b) the reweigh pass over the evaluated table, beside okx_ensemble_reduce (no factors) over the same table; a workgroup holds 8
      scenarios, so the table is walked once per scenario tile - reported as (scenario tiles x table bytes) over the kernel time, as a
      share of the 8 TB/s HBM peak, beside the fp64 operations per second (15 per state and scenario, none of them fused) as a share
      of the 39.3e12 the vector units retire (the datasheet's 78.6 TFLOP/s counts a fused multiply-add as two);
  (c) what the user must otherwise do: the table's .cpu() (timed alone), then ensemble_stats.reweigh_host (NumPy) - timed on the first
      --host-geometries geometries only (it is linear in them) and scaled.

Nobody had measured this pass; no target is fixed.  The device accumulator of those first geometries is compared with reweigh_host's:
COUNT equal, the sums within 2 (n + 1) u sum |term| of the host's own terms, n the geometries whose weight is not 0.

  python tools/ensemble_whatif_rate.py --out profiles/r24/ensemble_whatif_rate.json
"""

from __future__ import annotations

import statistics
import sys
import time

import ensemble_rate_common as common
from ensemble_effects_rate import build
from ensemble_rate_common import timed

U = 2.0 ** -53
HBM_PEAK = 8.0e12
FP64_OPS_PEAK = 39.3e12
OPS_PER_TERM = 15  # w w, four products and ten adds per (state, scenario)
SCENARIO_TILE = 8  # okx_tilt.hip kST


def scenarios(plan, n: int):
    """``n`` scenarios that tighten the first three latents to between 0.5 and 0.95 of their tolerance."""
    names = plan.factor_names()
    return [{name: dict(ratio=0.5 + 0.45 * i / max(1, n - 1)) for name in names[:3]} for i in range(n)]


def host_bounds(values, status, mask, weights, shift):
    """``[N, 10, S, K]``: 2 (n + 1) u sum |term| of the host's own terms, n the geometries whose weight is not 0 (COUNT: 0, it is exact)."""
    import numpy as np

    from open_kinematics_amd.ensemble_stats import REWEIGH_COUNT, REWEIGH_FIELDS, reweigh_scenario_terms, reweigh_terms

    ok, d, below, above, _ = reweigh_terms(values, status, mask, shift, None)
    out = np.zeros((weights.shape[1], REWEIGH_FIELDS) + d.shape[1:])
    for i in range(weights.shape[1]):
        live = weights[:, i] != 0.0
        out[i] = 2.0 * (int(live.sum()) + 1) * U * np.abs(reweigh_scenario_terms(ok[live], d[live], below[live], above[live], weights[live, i])).sum(axis=1)
        out[i, REWEIGH_COUNT] = 0.0
    return out


def measure_one(args, n_geom: int) -> list:
    import numpy as np
    import torch

    from open_kinematics_amd.dist import ShardedEnsemble
    from open_kinematics_amd.ensemble_sample import tilt_weights_host, tolerance_scenarios
    from open_kinematics_amd.ensemble_stats import REWEIGH_COUNT, reweigh_host

    device = torch.device("cuda:0")
    s, reps = args.steps_per_geometry, args.reps
    dp, plan, rel, columns = build(n_geom, s, device)
    k = len(columns)
    counts = [int(x) for x in args.scenarios.split(",")]
    pipe = ShardedEnsemble(dp, plan, rel, s, metric_columns=columns, reduce=True, factors="sampled", whatif=scenarios(plan, counts[0]), chain_len=1,
                           predictor=False)
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
    result = pipe.whatif()
    mid = s // 2
    chain = {"step_ms": {"first": first_step_ms, "second": step_ms}, "geometries": result.geometries,
             "camber_at_mid_sweep": [{"ratio": 0.5 + 0.45 * i / max(1, counts[0] - 1), "std": float(result.std[i, mid, 0]), "ess": float(result.ess[i, mid, 0]),
                                      "mean_weight": float(result.mean_weight[i])} for i in (0, counts[0] - 1)]}
    copy_ms = []
    for _ in range(max(1, reps // 4)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = table.cpu()
        copy_ms.append((time.perf_counter() - t0) * 1e3)
    few = min(n_geom, args.host_geometries)
    values = host.numpy().reshape(n_geom, s, k)[:few]
    st, fl, sh, lat = status.cpu().numpy().reshape(n_geom, s)[:few], flags.cpu().numpy()[:few], shift.cpu().numpy(), latents.cpu().numpy()[:few]
    racc = dp.reduce_ensemble(table, steps_per_geometry=s, status=status, shift=shift)
    out = []
    for n in counts:
        tilt = tolerance_scenarios(plan, scenarios(plan, n))
        prepared = dp.tilt_prepare(tilt)
        weights = dp.tilt_weights(latents, prepared)
        acc = dp.reweigh_ensemble(table, steps_per_geometry=s, weights=weights, status=status, mask=flags, shift=shift)
        runs = timed(reps=reps, passes={"weights": lambda: dp.tilt_weights(latents, prepared, out=weights),
                                        "reweigh": lambda: dp.reweigh_ensemble(table, steps_per_geometry=s, weights=weights, status=status, mask=flags, out=acc),
                                        "reduce": lambda: dp.reduce_ensemble(table, steps_per_geometry=s, status=status, out=racc)})
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_weights = tilt_weights_host(lat, tilt)
        want = reweigh_host(values, st, fl, host_weights, sh)
        host_ms = (time.perf_counter() - t0) * 1e3
        got = dp.reweigh_ensemble(table[: few * s], steps_per_geometry=s, weights=weights[:few], status=status[: few * s], mask=flags[:few], shift=shift).numpy().acc
        bound = host_bounds(values, st, fl, host_weights, sh)
        tiles = (n + SCENARIO_TILE - 1) // SCENARIO_TILE
        seconds = runs["reweigh"]["median"] * 1e-6
        out.append({
            "workload": f"C5 sampled (LHS): {n_geom} geometries x {s} steps, {k} metric columns, {n} scenarios tightening 3 of 30 latents, one GPU",
            "a_weights_us": runs["weights"],
            "b_reweigh_us": runs["reweigh"],
            "b_reduce_us": runs["reduce"],
            "reweigh_over_reduce": runs["reweigh"]["median"] / runs["reduce"]["median"],
            "table_bytes": table_bytes,
            "scenario_tiles": tiles,
            "tile_traffic_bytes_per_s": tiles * table_bytes / seconds,
            "tile_traffic_share_of_hbm_peak": tiles * table_bytes / seconds / HBM_PEAK,
            "fp64_operations_per_s": OPS_PER_TERM * n * n_geom * s * k / seconds,
            "fp64_share_of_vector_peak": OPS_PER_TERM * n * n_geom * s * k / seconds / FP64_OPS_PEAK,
            "scratch_bytes": int(dp.lib.okx_ensemble_reweigh_scratch_bytes(n_geom, s, k, n)),
            "c_host_path_ms": {"copy_alone_median": statistics.median(copy_ms), "copy_runs": copy_ms, "host_geometries": few,
                               "tilt_weights_host_and_reweigh_host": host_ms, "scaled_to_the_table": host_ms * n_geom / few},
            "weights_equal_the_host_bit_for_bit": bool(np.array_equal(weights[:few].cpu().numpy().view(np.uint64), host_weights.view(np.uint64))),
            "count_equals_reweigh_host": bool(np.array_equal(got[:, REWEIGH_COUNT], want.acc[:, REWEIGH_COUNT])),
            "device_within_bound_of_reweigh_host": bool(np.all(np.abs(got - want.acc) <= bound)),
            "largest_difference_over_bound": float(np.max(np.abs(got - want.acc) / np.where(bound > 0, bound, 1.0))),
            "chain": chain if n == counts[0] else None,
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
        a, b, rd, h = r["a_weights_us"], r["b_reweigh_us"], r["b_reduce_us"], r["c_host_path_ms"]
        lines.append(r["workload"])
        lines.append(f"(a) weights {a['median']:10.1f} us (interquartile {a['interquartile']:.1f})")
        lines.append(f"(b) reweigh {b['median']:10.1f} us (interquartile {b['interquartile']:.1f})   reduce, same table {rd['median']:9.1f} us   ratio "
                     f"{r['reweigh_over_reduce']:.2f}   {r['scenario_tiles']} scenario tiles x {r['table_bytes'] / 1e6:.0f} MB: "
                     f"{r['tile_traffic_bytes_per_s'] / 1e12:.2f} TB/s = {r['tile_traffic_share_of_hbm_peak']:.2f} of the HBM peak;   "
                     f"{r['fp64_operations_per_s'] / 1e12:.2f}e12 fp64 operations/s = {r['fp64_share_of_vector_peak']:.2f} of the vector peak")
        lines.append(f"(c) host route: copy alone {h['copy_alone_median']:.1f} ms, then tilt_weights_host + reweigh_host {h['scaled_to_the_table']:.0f} ms "
                     f"(timed on {h['host_geometries']} geometries: {h['tilt_weights_host_and_reweigh_host']:.0f} ms);   weights equal: "
                     f"{r['weights_equal_the_host_bit_for_bit']}, COUNT equal: {r['count_equals_reweigh_host']}, sums within 2 (n + 1) u sum |term|: "
                     f"{r['device_within_bound_of_reweigh_host']} (largest {r['largest_difference_over_bound']:.3f} of the bound)")
        if r["chain"]:
            c = r["chain"]
            ends = ", ".join(f"ratio {t['ratio']:.2f}: std {t['std']:.4g}, ess {t['ess']:.0f}, mean weight {t['mean_weight']:.3f}" for t in c["camber_at_mid_sweep"])
            lines.append(f"    chain step (rebind, evaluated solve, reduce, reweigh): {c['step_ms']['second']:.1f} ms; camber at mid sweep, {ends}")
    return "\n".join(lines) + "\n"


def main() -> int:
    ap = common.parser(rehearsal=False, steps_per_geometry=256, reps=20, host_geometries=1024)
    ap.add_argument("--geometries", default="4096,131072", help="the ensemble sizes to measure")
    ap.add_argument("--scenarios", default="8,64", help="the scenario counts to measure")
    return common.run(ap.parse_args(), measure, summary)


if __name__ == "__main__":
    sys.exit(main())
