"""
What drawing an ensemble on device costs (okx_ensemble_sample, DeviceProgram.sample_ensemble) on ONE GPU, device events, 20
repetitions after warm-up, all in one run and alternated block by block so that a drift hits every variant alike:

  (a) the pass for BASELINE config 5's plan (workloads.ensemble_plan: 15 points, 30 perturbed coordinates, the loader's two
      validators as guards, up to 16 attempts) at G = 4096 and G = 262144, IID and LHS, without and with a dense 30 x 30
      mixing - hardpoints and flags written, then the same with the latents and deltas too;
  (b) the host route the pass replaces: workloads.ensemble_problem's sequential NumPy draw (one generator, invalid geometries
      redrawn in order) RESTATED in this tool so that only the draw is timed, not the YAML load - the run checks that the
      restated loop returns ensemble_problem's own table, a function this change leaves as it was - plus the upload of the
      same table (torch.as_tensor(table, device=...), synchronised).

The expectation recorded with the pass was that the table write bounds it (C5: 4096 x 45 doubles = 1.5 MB); the bytes written
per second are in the output either way.  No test asserts a time.

  python tools/ensemble_sample_rate.py --out profiles/r17/ensemble_sample_rate.json
"""

from __future__ import annotations

import statistics
import sys
import time

import ensemble_rate_common as common
from ensemble_rate_common import alternated, spread


def host_route(program, plan, n_geometries: int, sigma: float, seed: int):
    """``ensemble_problem``'s draw: every authored coordinate + N(0, sigma), one generator, invalid geometries redrawn in sequence."""
    import numpy as np

    from open_kinematics_amd.ensemble_sample import GUARD_OFF_LINE, GUARD_SIGN

    sign = [g for g in plan.guards if g[0] == GUARD_SIGN][0]
    line = [g for g in plan.guards if g[0] == GUARD_OFF_LINE][0]
    outboard, anchors, eps = sign[1] // 3, list(line[1:4]), line[4]
    authored = sorted({int(c) // 3 for c in plan.coords})

    def valid(points) -> bool:
        if points[outboard, 1] <= 0.0:
            return False
        a, b, c = points[anchors]
        span = float(np.linalg.norm(b - a))
        if span <= eps:
            return False
        return float(np.linalg.norm(np.cross(c - a, (b - a) / span))) > eps

    rng = np.random.default_rng(seed)
    table = np.repeat(program.design_pos[None], n_geometries, axis=0)
    g = 0
    while g < n_geometries:
        trial = program.design_pos.copy()
        trial[authored] += rng.normal(0.0, sigma, (len(authored), 3))
        if not valid(trial):
            continue
        table[g] = trial
        g += 1
    return table


def measure(args) -> dict:
    import numpy as np
    import torch

    from open_kinematics_amd.batch import DeviceProgram
    from open_kinematics_amd.ensemble_sample import IID, LHS, SamplePlan, sample_host
    from open_kinematics_amd.workloads import ensemble_plan

    device = torch.device("cuda:0")
    sizes = [int(g) for g in args.geometries.split(",")]
    reps = args.reps
    dp = None
    variants, plans, program = {}, {}, None
    for g in sizes:
        for stratify, word in ((IID, "iid"), (LHS, "lhs")):
            program, plan, _ = ensemble_plan(g, args.sigma, args.seed, n_steps=4, stratify=stratify)
            if dp is None:
                dp = DeviceProgram(program, device)
            f = plan.n_coords
            mixing = np.random.default_rng(7).normal(0.0, args.sigma / np.sqrt(f), (f, f))
            mixed = SamplePlan(plan.nominal, plan.coords, plan.kind, plan.bound, mixing, None, stratify, g, args.seed, plan.guards, plan.max_attempts)
            for name, p in ((f"g{g}_{word}", plan), (f"g{g}_{word}_mixing", mixed)):
                plans[name] = p
                for full in (False, True):
                    out = dp.sample_ensemble(p, latents=full, delta=full)
                    variants[name + ("_all_outputs" if full else "")] = (p, out)
    torch.cuda.synchronize()

    passes = {name: (lambda p=p, out=out: dp.sample_ensemble(p, out=out)) for name, (p, out) in variants.items()}
    runs = alternated(passes, reps, warm=max(1, args.warmup))
    device_us = {}
    for name, (p, out) in variants.items():
        n = int(out.hardpoints.shape[0])
        written = n * (8 * p.n_points * 3 + 1 + (8 * (p.n_latents + p.n_coords) if out.latents is not None else 0))
        med = statistics.median(runs[name])
        flags = out.flags.cpu().numpy()
        device_us[name] = {"geometries": n, "median": med, "interquartile": spread(runs[name]), "bytes_written": written,
                           "written_gb_per_s": written / (med * 1e-6) / 1e9, "geometries_per_s": n / (med * 1e-6),
                           "redrawn": int((flags >> 4 > 0).sum()), "flagged": int((flags & 1).sum()), "runs": runs[name]}
    # the device's bits against the definition, the first and the last 128 geometries of every plan
    equal = {}
    for name, p in plans.items():
        _, out = variants[name + "_all_outputs"]
        n = int(out.hardpoints.shape[0])
        ok = True
        for lo, hi in ((0, min(128, n)), (max(0, n - 128), n)):
            want = sample_host(p, lo, hi)
            got = [t[lo:hi].cpu().numpy() for t in (out.hardpoints, out.latents, out.delta)]
            ok = ok and all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(got, want[:3]))
            ok = ok and np.array_equal(out.flags[lo:hi].cpu().numpy(), want[3])
        equal[name] = bool(ok)

    # (b) the host route: the sequential draw, then the upload of its table
    host = {}
    for g in sizes:
        plan = plans[f"g{g}_iid"]
        draws = []
        for _ in range(3 if g <= 8192 else 1):
            t0 = time.perf_counter()
            table = host_route(program, plan, g, args.sigma, args.seed)
            draws.append((time.perf_counter() - t0) * 1e3)
        uploads = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            torch.as_tensor(table, device=device)
            torch.cuda.synchronize()
            uploads.append((time.perf_counter() - t0) * 1e3)
        if g <= 8192:  # the restated loop IS ensemble_problem's: the same table
            from open_kinematics_amd.workloads import ensemble_problem

            restated_equals = bool(np.array_equal(table, ensemble_problem(g, 4, args.sigma, args.seed)[1]))
        host[f"g{g}"] = {"geometries": g, "equals_ensemble_problem": restated_equals if g <= 8192 else None,
                         "draw_ms_median": statistics.median(draws), "draw_runs_ms": draws,
                         "upload_ms_median": statistics.median(uploads), "upload_interquartile_ms": spread(uploads), "table_bytes": int(table.nbytes)}
    plan = plans[f"g{sizes[0]}_iid"]
    return {
        "workload": f"C5's plan: {plan.n_points} points, {plan.n_coords} perturbed coordinates, sigma {args.sigma}, {len(plan.guards)} guards, "
                    f"up to {plan.max_attempts} attempts; one GPU",
        "a_device_pass_us": device_us,
        "device_equals_sample_host": equal,
        "b_host_route_restated_from_ensemble_problem": host,
    }


def summary(r: dict) -> str:
    lines = [r["workload"]]
    for name, c in r["a_device_pass_us"].items():
        lines.append(f"(a) {name:<34} {c['median']:9.1f} us  (interquartile {c['interquartile']:.1f})   {c['written_gb_per_s']:7.1f} GB/s written   "
                     f"{c['geometries_per_s'] / 1e6:8.1f} M geometries/s   {c['redrawn']} redrawn, {c['flagged']} flagged")
    lines.append("    device == sample_host (first and last 128 geometries, all four outputs): " + ", ".join(f"{k}: {v}" for k, v in r["device_equals_sample_host"].items()))
    for name, h in r["b_host_route_restated_from_ensemble_problem"].items():
        lines.append(f"(b) {name:<10} restated sequential NumPy draw {h['draw_ms_median']:.1f} ms, upload of its {h['table_bytes']} bytes {h['upload_ms_median'] * 1e3:.1f} us "
                     f"(interquartile {h['upload_interquartile_ms'] * 1e3:.1f})")
    return "\n".join(lines) + "\n"


def main() -> int:
    ap = common.parser(rehearsal=False)
    ap.add_argument("--geometries", default="4096,262144")
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    return common.run(ap.parse_args(), measure, summary)


if __name__ == "__main__":
    sys.exit(main())
