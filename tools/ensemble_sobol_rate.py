"""
What the Sobol' chain costs (okx_ensemble_sample_families, okx_ensemble_sobol) on BASELINE config 5's shape - 4096 pick-freeze
families of the perturbed double wishbone x 256 bump steps, bench.py's four metric columns - for D = 10 (the latents grouped by
point, 49 152 geometries) and D = 30 (one group per coordinate, 131 072 geometries), on ONE GPU, device events, 20 repetitions
after warm-up, alternated block by block so that a drift hits every pass alike:

  (a) the family draw, beside okx_ensemble_sample of the same row count;
  (b) the estimator pass over the evaluated table, beside okx_ensemble_reduce (no factors) over the same table, and the table's
      bytes / pass time;
  (c) what the user must otherwise do: the table's .cpu() (timed alone), then ensemble_stats.sobol_host (NumPy).

Nobody had measured this pass; no target is fixed.  The device accumulator is compared with sobol_host's within the summation
bound 2 (n + 1) u sum |term| of its own terms.

  python tools/ensemble_sobol_rate.py --out profiles/r19/ensemble_sobol_rate.json

``--rehearse N``: N ranks on cuda:0 over gloo (fresh child processes), each running ShardedEnsemble(reduce=True, sobol=True) in two
chunks and writing its merged Sobol' accumulator to ``<out>/rank<r>.pt`` - once over the evaluated table and once more with the
Sobol stage fed an INTEGER table (``integer_rows``) in its place, whose sums are exact (tests/test_gpu_ensemble_sobol.py).
"""

from __future__ import annotations

import dataclasses
import os
import statistics
import sys
import time

import ensemble_rate_common as common
from ensemble_rate_common import rank, timed


U = 2.0 ** -53


def build(n_families: int, steps: int, device, *, by_point: bool = True, n_points=None, stratify: int = 1):
    from open_kinematics_amd.batch import DeviceProgram
    from open_kinematics_amd.input import load_geometry
    from open_kinematics_amd.metrics import corner_roles
    from open_kinematics_amd.workloads import ensemble_family_plan, geometry_path

    program, fplan, rel = ensemble_family_plan(n_families, 1.0, 3, n_steps=steps, n_points=n_points, by_point=by_point, stratify=stratify)
    dp = DeviceProgram(program, device)
    dp.enable_evaluation(corner_roles(load_geometry(geometry_path("geometry.yaml")), program))
    bump = program.n_targets - 1
    columns = [("camber", None), ("camber", bump), ("roadwheel_angle", bump), (21, bump)]
    return dp, fplan, rel, columns


def integer_rows(lo: int, hi: int, n_columns: int):
    """Rows ``[lo, hi)`` of the rehearsal's integer table ``[rows, K]`` (values in [-8, 8], a function of the global row and the column
    alone) and their status bytes (every 37th row rejected), NumPy."""
    import numpy as np

    r = np.arange(lo, hi, dtype=np.int64)[:, None]
    c = np.arange(n_columns, dtype=np.int64)[None]
    values = ((r * (2 * c + 3) + 5 * c + (r * r) % 11) % 17 - 8).astype(np.float64)
    status = np.where(r[:, 0] % 37 == 36, 2, 1).astype(np.uint8)
    return values, status


def rank_main(args) -> None:
    import numpy as np
    import torch

    from open_kinematics_amd.dist import ShardedEnsemble

    with rank(args) as device:
        s = args.steps_per_geometry
        dp, fplan, rel, columns = build(args.families, s, device, n_points=args.points or None)
        k = len(columns)
        pipe = ShardedEnsemble(dp, fplan, rel, s, metric_columns=columns, reduce=True, sobol=True, chunks=2, shift=np.zeros((s, k)), chain_len=1,
                               predictor=False)
        pipe.step()
        torch.cuda.synchronize()
        real = pipe.sobol_accumulator.acc.cpu().clone()
        # the Sobol stage once more, its chunks fed the integer table in place of the evaluated one
        glo, ghi = pipe.geometry_range
        values, status = integer_rows(glo * s, ghi * s, k)
        pipe.metric_local.copy_(torch.as_tensor(values, device=device))
        pipe.info_local[:, 32] = torch.as_tensor(status, device=device)
        stage = pipe.stages["sobol"]
        stage.begin_step()
        for c in range(pipe.chunks):
            a, b = pipe.pieces[c][pipe.rank]
            if b > a:
                stage.rows(a, b, slice((a - glo) * s, (b - glo) * s))
        stage.end_step()
        torch.cuda.synchronize()
        torch.save({"acc": real, "integer_acc": pipe.sobol_accumulator.acc.cpu().clone(), "flags": pipe.sampled_flags.cpu(), "range": pipe.geometry_range,
                    "pieces": pipe.pieces, "sent": pipe.sobol_exchange_bytes_per_rank}, os.path.join(args.out, f"rank{args.rank}.pt"))


def rehearse(args) -> int:
    return common.rehearse(args, __file__, 36500, ["--families", args.families, "--steps-per-geometry", args.steps_per_geometry,
                                                        "--points", args.points])


def measure_one(args, by_point: bool) -> dict:
    import numpy as np
    import torch

    from open_kinematics_amd.dist import ShardedEnsemble
    from open_kinematics_amd.ensemble_stats import sobol_host, sobol_terms

    device = torch.device("cuda:0")
    n, s = args.families, args.steps_per_geometry
    dp, fplan, rel, columns = build(n, s, device, by_point=by_point)
    d, m, k = fplan.n_groups, fplan.family_size, len(columns)
    g = n * m
    reps = args.reps

    # (a) the draw
    plain = dataclasses.replace(fplan.plan, n_total=g)
    fam_out, plain_out = dp.sample_families(fplan), dp.sample_ensemble(plain)
    draw = timed(reps=reps, passes={"sample_families": lambda: dp.sample_families(fplan, out=fam_out), "sample_ensemble": lambda: dp.sample_ensemble(plain, out=plain_out)})
    del fam_out, plain_out
    # (b) the estimator over the evaluated table
    pipe = ShardedEnsemble(dp, fplan, rel, s, metric_columns=columns, reduce=True, sobol=True, chain_len=1, predictor=False)
    t0 = time.perf_counter()
    pipe.step()
    torch.cuda.synchronize()
    first_step_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    pipe.step()
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t0) * 1e3
    table, status, flags = pipe.metric_local, pipe.info_local[:, 32], pipe.sampled_flags
    shift = pipe.local_accumulator.shift
    acc = dp.sobol_ensemble(table, steps_per_geometry=s, n_groups=d, status=status, mask=flags, shift=shift)
    racc = dp.reduce_ensemble(table, steps_per_geometry=s, status=status, shift=shift)
    est = timed(reps=reps, passes={"sobol": lambda: dp.sobol_ensemble(table, steps_per_geometry=s, n_groups=d, status=status, mask=flags, out=acc),
                 "reduce": lambda: dp.reduce_ensemble(table, steps_per_geometry=s, status=status, out=racc)})
    torch.cuda.synchronize()
    table_bytes = 8 * g * s * k
    # (c) the host route
    copy_ms = []
    for _ in range(max(1, reps // 4)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = table.cpu()
        copy_ms.append((time.perf_counter() - t0) * 1e3)
    values = host.numpy().reshape(g, s, k)
    st, fl, sh = status.cpu().numpy().reshape(g, s), flags.cpu().numpy(), shift.cpu().numpy()
    t0 = time.perf_counter()
    want = sobol_host(values, st, fl, d, sh)
    host_ms = (time.perf_counter() - t0) * 1e3
    got = acc.numpy().acc
    bound = np.zeros_like(got)
    for lo in range(0, g, 64 * m):  # 2 (n + 1) u sum |term| of the host's own terms
        rows = slice(lo, lo + 64 * m)
        bound += np.abs(sobol_terms(values[rows], st[rows], fl[rows], d, sh)[1]).sum(axis=0)
    bound *= 2.0 * (n + 1) * U
    result = pipe.sobol()
    mid = s // 2
    return {
        "workload": f"C5 pick-freeze: {n} families x M = {m} (D = {d}) = {g} geometries x {s} steps, {k} metric columns, one GPU",
        "a_draw_us": draw,
        "b_estimator_us": est,
        "sobol_over_reduce": est["sobol"]["median"] / est["reduce"]["median"],
        "table_bytes": table_bytes,
        "table_bytes_per_s": table_bytes / (est["sobol"]["median"] * 1e-6),
        "chain_step_ms": {"first": first_step_ms, "second": step_ms},
        "c_host_path_ms": {"copy_alone_median": statistics.median(copy_ms), "copy_runs": copy_ms, "sobol_host": host_ms},
        "device_within_bound_of_sobol_host": bool(np.all(np.abs(got - want.acc) <= bound)),
        "largest_difference_over_bound": float(np.max(np.abs(got - want.acc) / np.where(bound > 0, bound, 1.0))),
        "families_counted_min_max": [int(result.count.min()), int(result.count.max())],
        "camber_at_mid_sweep": {"groups": result.group_names, "first": [float(x) for x in result.first[mid, 0]], "total": [float(x) for x in result.total[mid, 0]]},
    }


def measure(args) -> list:
    return [measure_one(args, by_point=which == "10") for which in args.groups.split(",")]


def summary(results: list) -> str:
    lines = []
    for r in results:
        lines.append(r["workload"])
        a, b, h = r["a_draw_us"], r["b_estimator_us"], r["c_host_path_ms"]
        lines.append(f"(a) sample_families {a['sample_families']['median']:9.1f} us (interquartile {a['sample_families']['interquartile']:.1f})   "
                     f"sample_ensemble, same rows {a['sample_ensemble']['median']:9.1f} us")
        lines.append(f"(b) sobol           {b['sobol']['median']:9.1f} us (interquartile {b['sobol']['interquartile']:.1f})   reduce, same table "
                     f"{b['reduce']['median']:9.1f} us   ratio {r['sobol_over_reduce']:.2f}   {r['table_bytes'] / 1e6:.0f} MB at {r['table_bytes_per_s'] / 1e12:.2f} TB/s")
        lines.append(f"(c) host route: copy alone {h['copy_alone_median']:.1f} ms, then sobol_host {h['sobol_host']:.0f} ms;   "
                     f"device within 2 (n + 1) u sum |term| of it: {r['device_within_bound_of_sobol_host']} (largest {r['largest_difference_over_bound']:.3f} of the bound)")
        lines.append(f"    chain step (draw was before; rebind, evaluated solve, reduce, sobol): {r['chain_step_ms']['second']:.1f} ms; families counted per entry "
                     f"{r['families_counted_min_max'][0]} .. {r['families_counted_min_max'][1]}")
    return "\n".join(lines) + "\n"


def main() -> int:
    ap = common.parser(families=4096, steps_per_geometry=256, timeout=600.0)
    ap.add_argument("--points", type=int, default=0, help="perturb the first POINTS authored points only (0: all)")
    ap.add_argument("--groups", default="10,30", help="which groupings to measure: 10 (by point) and / or 30 (by coordinate)")
    ap.add_argument("--reps", type=int, default=20)
    return common.run(ap.parse_args(), measure, summary, rank_main, rehearse)


if __name__ == "__main__":
    sys.exit(main())
