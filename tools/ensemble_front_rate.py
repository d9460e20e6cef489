"""
What the on-device Pareto front costs (okx_ensemble_front, DeviceProgram.front_ensemble) on BASELINE config 5 - 4096 perturbed
geometries x 256 bump steps, bench.py's four metric columns - on ONE GPU, device events, 20 repetitions after warm-up, all in one
run and alternated block by block so that a drift hits every pass alike:

  (a) the front pass for M = 2, 4 and 8 objectives over the curve-feature table [4096, 4 * 12] that okx_ensemble_curves left in
      HBM (gradients, curvatures and extremes of the four columns), with the screen's flag bytes as its mask;
  (b) on the same table: okx_ensemble_screen - a pass that reads the table once;
  (c) what the user must otherwise do: the table's .cpu() (timed alone), then ensemble_stats.front_host (NumPy, O(G^2 M)).

The pass is 1.7e7 pair tests of M objectives: little work, three short launches.  Nobody had measured it; the expectation -
recorded, not a gate - was tens of microseconds.  The ratio to the screen pass is in the output either way.

  python tools/ensemble_front_rate.py --out profiles/r16/ensemble_front_rate.json
"""

from __future__ import annotations

import statistics
import sys
import time

import ensemble_rate_common as common
from ensemble_rate_common import alternated, spread
from ensemble_curves_rate import curve_arguments
from ensemble_reduce_rate import build


def front_objectives(n_columns: int, m: int) -> list:
    """M objectives over the feature table: per column the gradient at the origin (towards 0), then the curvature (small), then
    the extremes - entry ``column * 12 + field`` of the one step."""
    from open_kinematics_amd.ensemble_stats import CURVE_C1, CURVE_C2, CURVE_FIELDS, CURVE_MAX, CURVE_MIN

    picks = [(c, CURVE_C1, "target", 0.0) for c in range(n_columns)] + [(c, CURVE_C2, "min") for c in range(n_columns)]
    picks += [(c, f, sense) for c in range(n_columns) for f, sense in ((CURVE_MAX, "min"), (CURVE_MIN, "max"))]
    return [(0, c * CURVE_FIELDS + f) + tuple(rest) for c, f, *rest in picks[:m]]


def measure(args) -> dict:
    import numpy as np
    import torch

    from open_kinematics_amd.dist import ShardedEnsemble
    from open_kinematics_amd.ensemble_stats import CURVE_C1, CURVE_FIELDS, front_host

    device = torch.device("cuda:0")
    g, s = args.geometries, args.steps_per_geometry
    dp, table, rel, columns = build(g, s, device)
    k = len(columns)
    reduced = ShardedEnsemble(dp, table, rel, s, metric_columns=columns, reduce=True, chain_len=1, predictor=False)
    for _ in range(max(1, args.warmup)):
        reduced.step()
    torch.cuda.synchronize()
    curves = dp.curves_ensemble(reduced.metric_local, steps_per_geometry=s, status=reduced.info_local[:, 32], **curve_arguments(rel, 2))
    features = curves.table()  # [G, K * 12], one step per geometry
    n = k * CURVE_FIELDS
    torch.cuda.synchronize()
    # the screen: the 5 % - 95 % band of the camber gradient; everything else is not looked at
    gradient = features[:, CURVE_C1].cpu().numpy()
    limits = np.full((1, n, 2), (-np.inf, np.inf))
    limits[0, CURVE_C1] = np.nanquantile(gradient, 0.05), np.nanquantile(gradient, 0.95)
    scr = dp.screen_ensemble(features, steps_per_geometry=1, limits=limits)
    reps = args.reps

    passes, outs = {}, {}
    for m in (2, 4, 8):
        out = dp.front_ensemble(features, steps_per_geometry=1, objectives=front_objectives(k, m), mask=scr.flags)
        outs[m] = out
        passes[f"front_m{m}"] = lambda out=out: dp.front_ensemble(features, steps_per_geometry=1, mask=scr.flags, out=out)
    passes["screen"] = lambda: dp.screen_ensemble(features, steps_per_geometry=1, out=scr)
    runs = alternated(passes, reps)
    med = {name: statistics.median(r) for name, r in runs.items()}

    # (c) the host route: the copy alone, then front_host on the copied table
    copy_ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = features.cpu()
        copy_ms.append((time.perf_counter() - t0) * 1e3)
    mask = scr.flags.cpu().numpy()
    host_ms, equal, tallies = {}, {}, {}
    for m, out in outs.items():
        t0 = time.perf_counter()
        want = front_host(host.numpy()[:, None, :], None, front_objectives(k, m), mask)
        host_ms[m] = (time.perf_counter() - t0) * 1e3
        got = out.finalize()
        equal[m] = bool(np.array_equal(got.dominated, want.dominated) and np.array_equal(got.tally, want.tally) and np.array_equal(got.index, want.index)
                        and np.array_equal(got.values.view(np.uint64), want.values.view(np.uint64)))
        tallies[m] = [int(x) for x in want.tally]
    fronts = {name: {"objectives": int(name[7:]), "median": med[name], "interquartile": spread(runs[name]), "over_screen": med[name] / med["screen"],
                     "pair_tests_per_s": g * g / (med[name] * 1e-6), "seen_candidates_members": tallies[int(name[7:])], "runs": runs[name]}
              for name in passes if name.startswith("front")}
    return {
        "workload": f"C5: {g} geometries x {s} steps, {k} metric columns -> the curve-feature table [{g}, {n}], one GPU",
        "a_front_pass_us": fronts,
        "b_same_table_us": {"screen": {"median": med["screen"], "interquartile": spread(runs["screen"]), "runs": runs["screen"]}},
        "expectation_tens_of_microseconds": {"largest_median_us": max(f["median"] for f in fronts.values()),
                                             "holds": bool(max(f["median"] for f in fronts.values()) < 100.0)},
        "c_host_path_ms": {"copy_alone_median": statistics.median(copy_ms), "copy_runs": copy_ms, "front_host": {str(m): t for m, t in host_ms.items()}},
        "device_equals_front_host": {str(m): e for m, e in equal.items()},
        "table_bytes": 8 * g * n,
    }


def summary(r: dict) -> str:
    lines = [r["workload"]]
    for name, c in r["a_front_pass_us"].items():
        seen, candidates, members = c["seen_candidates_members"]
        lines.append(f"(a) {name:<10} {c['median']:8.1f} us  (interquartile {c['interquartile']:.1f})   / screen = {c['over_screen']:.2f}   "
                     f"{c['pair_tests_per_s'] / 1e12:.2f} T pair tests/s   {candidates} candidates of {seen}, {members} on the front")
    c = r["b_same_table_us"]["screen"]
    lines.append(f"(b) {'screen':<10} {c['median']:8.1f} us  (interquartile {c['interquartile']:.1f})")
    e, h = r["expectation_tens_of_microseconds"], r["c_host_path_ms"]
    lines.append(f"    expectation, tens of microseconds: largest median {e['largest_median_us']:.1f} us - " + ("holds" if e["holds"] else "MISSED"))
    lines.append(f"(c) copy alone {h['copy_alone_median'] * 1e3:.1f} us, then front_host " + ", ".join(f"M = {m}: {t:.1f} ms" for m, t in h["front_host"].items()))
    lines.append("    device == front_host (dominated, tally, ids, value bits): " + ", ".join(f"M = {m}: {e}" for m, e in r["device_equals_front_host"].items()))
    return "\n".join(lines) + "\n"


def main() -> int:
    ap = common.parser(geometries=4096, steps_per_geometry=256, warmup=3, reps=20, rehearsal=False)
    return common.run(ap.parse_args(), measure, summary)


if __name__ == "__main__":
    sys.exit(main())
