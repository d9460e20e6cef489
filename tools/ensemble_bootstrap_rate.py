"""
What the bootstrap of the Sobol' indices costs (okx_ensemble_sobol_bootstrap, okx_ensemble_bootstrap_weights) on BASELINE config 5's
shape - the evaluated table of tools/ensemble_sobol_rate.py: 4096 pick-freeze families of the perturbed double wishbone x 256 bump
steps, bench.py's four metric columns, D = 10 and D = 30 - for R = 64 and R = 256 replicates, on ONE GPU, device events, 20
repetitions after warm-up, alternated block by block so that a drift hits every pass alike:

  (a) the new pass, beside okx_ensemble_sobol over the same table in the same run (T_base: the existing kernel, untouched);
  (b) the weights kernel alone (the [4096, R] table the public entry point writes);
  (c) what the user must otherwise do first: the table's .cpu(), timed alone.

THE CONDITION: the pass for R replicates must take less than R x T_base - what R passes through the existing entry point would cost
at the very least, before anyone builds the R reweighted tables.  ``condition_holds`` says so per (D, R); the ratio
pass / (R x T_base) stands beside it.  Beside the times: the fp64 operations the pass needs (2 per weighted term and replicate that
is drawn, P(w > 0) = 1 - 1/e of them, from the sizes) and the table bytes it must read at least once, over the pass time.

Checked in the same run: COUNT_r + DROPPED_r equals the weight sums exactly in every entry, and the first 16 families agree with
ensemble_stats.sobol_bootstrap_host exactly in the integer fields and within 2 (n + 1) u sum |w term| in the others.

  python tools/ensemble_bootstrap_rate.py --out profiles/r21/ensemble_bootstrap_rate.json
"""

from __future__ import annotations

import math
import statistics
import sys

import ensemble_rate_common as common
from ensemble_rate_common import timed


U = 2.0 ** -53
PEAK_FP64_VECTOR = 78.6e12   # MI355X datasheet, FLOP/s
PEAK_HBM = 8.0e12            # datasheet, B/s


def measure_one(args, by_point: bool, replicates: list) -> dict:
    import numpy as np
    import torch

    from ensemble_sobol_rate import build
    from open_kinematics_amd.dist import ShardedEnsemble
    from open_kinematics_amd.ensemble_stats import SOBOL_COUNT, SOBOL_DROPPED, bootstrap_weights, sobol_bootstrap_host, sobol_terms

    device = torch.device("cuda:0")
    n, s = args.families, args.steps_per_geometry
    dp, fplan, rel, columns = build(n, s, device, by_point=by_point)
    d, m, k = fplan.n_groups, fplan.family_size, len(columns)
    g = n * m
    seed = fplan.plan.seed

    pipe = ShardedEnsemble(dp, fplan, rel, s, metric_columns=columns, reduce=True, sobol=True, chain_len=1, predictor=False)
    pipe.step()
    torch.cuda.synchronize()
    table, status, flags = pipe.metric_local, pipe.info_local[:, 32], pipe.sampled_flags
    shift = pipe.local_accumulator.shift
    table_kw = dict(steps_per_geometry=s, n_groups=d, status=status, mask=flags)
    base = dp.sobol_ensemble(table, shift=shift, **table_kw)
    boots = {r: dp.sobol_bootstrap_ensemble(table, n_replicates=r, seed=seed, shift=shift, **table_kw) for r in replicates}
    weights = {r: dp.bootstrap_weights(n, r, seed) for r in replicates}
    passes = {"sobol": lambda: dp.sobol_ensemble(table, out=base, **table_kw)}
    for r in replicates:
        passes[f"bootstrap_R{r}"] = lambda r=r: dp.sobol_bootstrap_ensemble(table, n_replicates=r, seed=seed, out=boots[r], **table_kw)
        passes[f"weights_R{r}"] = lambda r=r: dp.bootstrap_weights(n, r, seed, out=weights[r])
    times = timed(passes, args.reps)
    torch.cuda.synchronize()
    copy_ms = []
    for _ in range(max(1, args.reps // 4)):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        host = table.cpu()
        b.record()
        torch.cuda.synchronize()
        copy_ms.append(a.elapsed_time(b))
    # the checks: weight sums everywhere, the first families against the host definition
    few = min(n, args.check_families)
    values = host.numpy().reshape(g, s, k)[: few * m]
    st, fl, sh = status.cpu().numpy().reshape(g, s)[: few * m], flags.cpu().numpy()[: few * m], shift.cpu().numpy()
    t_base = times["sobol"]["median"]
    table_bytes = 8 * g * s * k
    rows = []
    for r in replicates:
        got = boots[r].numpy().acc
        w = bootstrap_weights(seed, 0, n, r)
        sums_ok = bool(np.array_equal(got[..., SOBOL_COUNT] + got[..., SOBOL_DROPPED], np.broadcast_to(w.sum(axis=0)[:, None, None].astype(np.float64), got.shape[:3])))
        part = dp.sobol_bootstrap_ensemble(table[: few * m * s], n_replicates=r, seed=seed, shift=shift, steps_per_geometry=s, n_groups=d,
                                           status=status[: few * m * s], mask=flags[: few * m])
        torch.cuda.synchronize()
        want = sobol_bootstrap_host(values, st, fl, d, sh, seed=seed, n_replicates=r).acc
        _, terms, _ = sobol_terms(values, st, fl, d, sh)
        bound = np.zeros_like(want)
        for i in range(few):
            bound += np.abs(w[i].astype(np.float64)[:, None, None, None] * terms[i][None])
        bound *= 2.0 * (few + 1) * U
        diff = np.abs(part.numpy().acc - want)
        t = times[f"bootstrap_R{r}"]["median"]
        drawn = 1.0 - math.exp(-1.0)
        flops = 2.0 * (6 + 3 * d) * r * drawn * n * s * k
        rows.append({
            "replicates": r,
            "bootstrap_us": t,
            "bootstrap_interquartile_us": times[f"bootstrap_R{r}"]["interquartile"],
            "weights_alone_us": times[f"weights_R{r}"]["median"],
            "r_times_t_base_us": r * t_base,
            "ratio_to_r_times_t_base": t / (r * t_base),
            "condition_holds": bool(t < r * t_base),
            "per_replicate_over_t_base": t / r / t_base,
            "fp64_flops_needed": flops,
            "fp64_flops_per_s": flops / (t * 1e-6),
            "share_of_fp64_vector_peak": flops / (t * 1e-6) / PEAK_FP64_VECTOR,
            "table_bytes_per_s_read_once": table_bytes / (t * 1e-6),
            "least_time_us": max(flops / PEAK_FP64_VECTOR, table_bytes / PEAK_HBM) * 1e6,
            "bound_by": "fp64" if flops / PEAK_FP64_VECTOR > table_bytes / PEAK_HBM else "HBM",
            "weight_sums_exact": sums_ok,
            "first_families_integer_fields_exact": bool(np.array_equal(part.numpy().acc[..., :2], want[..., :2])),
            "first_families_within_bound": bool(np.all(diff <= bound)),
            "largest_difference_over_bound": float(np.max(diff / np.where(bound > 0, bound, 1.0))),
            "scratch_bytes": int(dp.lib.okx_ensemble_sobol_bootstrap_scratch_bytes(n, d, s, k, r)),
        })
    out = boots[replicates[-1]].finalize()
    mid = s // 2
    return {
        "workload": f"C5 pick-freeze: {n} families x M = {m} (D = {d}) = {g} geometries x {s} steps, {k} metric columns, one GPU",
        "t_base_sobol_us": t_base,
        "t_base_interquartile_us": times["sobol"]["interquartile"],
        "table_bytes": table_bytes,
        "copy_to_host_ms": {"median": statistics.median(copy_ms), "runs": copy_ms},
        "replicate_counts": rows,
        "times_us": times,
        "camber_at_mid_sweep": {"groups": out.group_names, "first_std": [float(x) for x in out.first_std[mid, 0]],
                                "total_std": [float(x) for x in out.total_std[mid, 0]],
                                "first_interval": [[float(x) for x in side[mid, 0]] for side in out.interval("first")]},
    }


def measure(args) -> list:
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device and has no other path")
    replicates = [int(r) for r in args.replicates.split(",")]
    return [measure_one(args, by_point=which == "10", replicates=replicates) for which in args.groups.split(",")]


def summary(results: list) -> str:
    lines = []
    for res in results:
        lines.append(res["workload"])
        lines.append(f"    T_base (okx_ensemble_sobol) {res['t_base_sobol_us']:9.1f} us (interquartile {res['t_base_interquartile_us']:.1f});   table {res['table_bytes'] / 1e6:.0f} MB, "
                     f".cpu() alone {res['copy_to_host_ms']['median']:.1f} ms")
        for row in res["replicate_counts"]:
            lines.append(f"    R = {row['replicates']:4d}: bootstrap {row['bootstrap_us']:10.1f} us (interquartile {row['bootstrap_interquartile_us']:.1f})   "
                         f"R x T_base {row['r_times_t_base_us']:10.1f} us   ratio {row['ratio_to_r_times_t_base']:.3f}   condition holds: {row['condition_holds']}   "
                         f"weights alone {row['weights_alone_us']:.1f} us")
            lines.append(f"              {row['fp64_flops_per_s'] / 1e12:.2f} TFLOP/s fp64 ({100 * row['share_of_fp64_vector_peak']:.1f} % of the vector peak), table read once at "
                         f"{row['table_bytes_per_s_read_once'] / 1e12:.3f} TB/s; least time {row['least_time_us']:.0f} us ({row['bound_by']}-bound);   weight sums exact: "
                         f"{row['weight_sums_exact']}, first families within the bound: {row['first_families_within_bound']} "
                         f"(largest {row['largest_difference_over_bound']:.3f} of it, integer fields exact: {row['first_families_integer_fields_exact']})")
    return "\n".join(lines) + "\n"


def main() -> int:
    ap = common.parser(families=4096, steps_per_geometry=256, rehearsal=False)
    ap.add_argument("--groups", default="10,30", help="which groupings to measure: 10 (by point) and / or 30 (by coordinate)")
    ap.add_argument("--replicates", default="64,256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--check-families", type=int, default=16, help="families compared with the host definition")
    return common.run(ap.parse_args(), measure, summary, echo=False)


if __name__ == "__main__":
    sys.exit(main())
