"""
What the evaluation of a response surface costs (okx_ensemble_predict) on BASELINE config 5's plan - the perturbed double wishbone, LHS, 30
latents - on ONE GPU, device events, 20 repetitions after warm-up, alternated block by block so that a drift hits every contender alike:

  (a) the fused pass, DeviceProgram.predict_ensemble(out=), against the route the project had for the same table - basis_factors into a
      [G, T] table, torch.matmul, the shift and torch.where, as predict_surface does it, with every table uploaded beforehand - on
      G in {4096, 131072} x T in {66, 496} (10 and 30 of the latents, degree 2 with interactions) x N in {36, 1024}.  The coefficients are
      drawn (the time does not depend on their values); the two tables are compared.  The allocator's peak above what is held before the
      call is taken for both.  The CONDITION is at G = 131072: fused faster on all four shapes by more than the larger interquartile range.
  (b) ensemble_virtual.virtual_ensemble over --virtual-geometries geometries of the plan through a surface FITTED on the 4096 solved
      geometries of C5 (T = 66, N = 36; three quantiles, limits, screen): wall time, geometries / s, and the per-chunk device time of the
      sampler (whose hardpoint table the virtual draw does not need: written and ignored), the predict pass and each consumer, with the
      share of the whole each makes at its number of calls.
  (c) DeviceProgram.validate_surface of that fit over its 4096 geometries, host-timed (it ends in host reads).

  python tools/ensemble_predict_rate.py --out profiles/r26/ensemble_predict_rate.json
"""

from __future__ import annotations

import dataclasses
import sys
import time

import ensemble_rate_common as common
from ensemble_effects_rate import build
from ensemble_rate_common import timed


def surface_with(basis, coefficients, shift):
    import numpy as np

    from open_kinematics_amd.ensemble_stats import EnsembleSurface

    n = coefficients.shape[1]
    return EnsembleSurface(np.arange(n), 0, 0, basis, shift, coefficients, None, None)


def peak_above(fn) -> int:
    """The allocator's peak [bytes] during ``fn`` above what is allocated before it."""
    import torch

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def measure_shapes(args, dp, plan) -> list:
    import numpy as np
    import torch

    from open_kinematics_amd.ensemble_stats import surface_terms

    device = dp.device
    rng = np.random.default_rng(26)
    out = []
    for n_geom in (int(x) for x in args.geometries.split(",")):
        big = dataclasses.replace(plan, n_total=n_geom)
        latents = dp.sample_ensemble(big, 0, n_geom, latents=True).latents
        for p in (10, 30):
            basis = surface_terms(big, factors=list(range(p)))
            t = basis.n_terms
            rows = dp.basis_factors(latents, basis)
            for n in (36, 1024):
                c, shift = rng.normal(size=(t, n)), rng.normal(size=n)
                model = dp.upload_surface(surface_with(basis, c, shift))
                table = torch.empty((n_geom, n), dtype=torch.float64, device=device)
                valid = torch.empty(n_geom, dtype=torch.uint8, device=device)
                nan = torch.full((), float("nan"), dtype=torch.float64, device=device)

                def fused():
                    return dp.predict_ensemble(model, latents, out=table, valid=valid)[0]

                def torch_route():
                    dp.basis_factors(latents, out=rows)
                    product = model.shift[None, :] + torch.matmul(rows.phi, model.coefficients)
                    return torch.where(rows.valid[:, None] != 0, product, nan)

                runs = timed(reps=args.reps, passes={"fused": fused, "torch": torch_route})
                torch.cuda.synchronize()
                a, b = fused(), torch_route()
                gap = float((a - b).abs().max() / b.abs().max())
                del a, b
                peaks = {"fused": peak_above(fused), "torch": peak_above(torch_route)}
                margin = max(runs["fused"]["interquartile"], runs["torch"]["interquartile"])
                out.append({"workload": f"C5 plan (LHS, 30 latents): {n_geom} geometries, P = {p} latents used, T = {t} terms, N = {n} entries, one GPU",
                            "geometries": n_geom, "terms": t, "entries": n, "fused_us": runs["fused"], "torch_route_us": runs["torch"],
                            "fused_over_torch": runs["fused"]["median"] / runs["torch"]["median"], "margin_us": margin,
                            "fused_faster_by_more_than_the_margin": bool(runs["torch"]["median"] - runs["fused"]["median"] > margin),
                            "useful_fp64_flop_per_s": 2.0 * n_geom * t * n / (runs["fused"]["median"] * 1e-6),
                            "phi_table_bytes": 8 * n_geom * t, "peak_bytes_above_held": peaks, "largest_gap_relative_to_the_largest_value": gap})
                del table, model
            del rows
    return out


def measure_virtual(args, dp, plan, rel, columns) -> dict:
    import numpy as np
    import torch

    from open_kinematics_amd.dist import ShardedEnsemble
    from open_kinematics_amd.ensemble_device import EnsembleSample
    from open_kinematics_amd.ensemble_virtual import virtual_ensemble

    s, k = args.steps_per_geometry, len(columns)
    few_entries = [step * k + c for step in np.linspace(0, s - 1, 9).astype(int) for c in range(k)]  # 36 entries: nine steps of the sweep
    pipe = ShardedEnsemble(dp, plan, rel, s, metric_columns=columns, reduce=True, factors="sampled", surface=dict(factors=list(range(10)), entries=few_entries),
                           chain_len=1, predictor=False)
    pipe.step()
    torch.cuda.synchronize()
    fit = pipe.surface()
    model = dp.upload_surface(fit)
    n = fit.coefficients.shape[1]
    # (c) the leave-one-out check of the fit over its own geometries
    table, status, flags, latents = pipe.metric_local, pipe.info_local[:, 32], pipe.sampled_flags, pipe.my_factors
    check = dp.validate_surface(model, fit, latents, table, steps_per_geometry=s, status=status, mask=flags)
    validate_ms = common.step_ms(lambda: dp.validate_surface(model, fit, latents, table, steps_per_geometry=s, status=status, mask=flags), 5)
    # (b) the virtual ensemble
    total, chunk = int(args.virtual_geometries), int(args.chunk)
    big = dataclasses.replace(plan, n_total=total, seed=26)
    spread = np.sqrt(fit.variance) + 1e-12
    limits = np.stack([fit.shift - 3.0 * spread, fit.shift + 3.0 * spread], axis=1)
    probs = [0.0001, 0.5, 0.9999]
    virtual_ensemble(dp, model, big, 0, min(total, 2 * chunk), chunk=chunk, probs=probs, limits=limits, scale=spread, screen=True, verdicts=False)  # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run = virtual_ensemble(dp, model, big, chunk=chunk, probs=probs, limits=limits, scale=spread, screen=True, verdicts=False)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    # the parts, per chunk
    rows = min(chunk, total)
    sample = EnsembleSample(torch.empty((rows, big.n_points, 3), dtype=torch.float64, device=dp.device),
                            torch.empty((rows, big.n_latents), dtype=torch.float64, device=dp.device), None, torch.empty(rows, dtype=torch.uint8, device=dp.device))
    out = torch.empty((rows, n), dtype=torch.float64, device=dp.device)
    valid = torch.empty(rows, dtype=torch.uint8, device=dp.device)
    dp.sample_ensemble(big, 0, rows, latents=True, out=sample)
    dp.predict_ensemble(model, sample.latents, mask=sample.flags, out=out, valid=valid)
    acc = dp.reduce_ensemble(out, steps_per_geometry=1, shift=model.shift.reshape(1, n))
    sel = dp.select_prepare(1, n, probs, limits, rounds=True)
    dp.select_begin(sel)
    scr = dp.screen_prepare(1, n, limits, spread, rows)
    parts = timed(reps=args.reps, passes={
        "sample": lambda: dp.sample_ensemble(big, 0, rows, latents=True, out=sample),
        "predict": lambda: dp.predict_ensemble(model, sample.latents, mask=sample.flags, out=out, valid=valid),
        "reduce": lambda: dp.reduce_ensemble(out, steps_per_geometry=1, out=acc),
        "select_count": lambda: dp.select_count(sel, 0, out, steps_per_geometry=1),
        "screen": lambda: dp.screen_ensemble(out, steps_per_geometry=1, out=scr, first_row=0)})
    chunks, rounds = -(-total // chunk), dp.select_rounds
    calls = {"sample": chunks * rounds, "predict": chunks * rounds, "reduce": chunks, "select_count": chunks * rounds, "screen": chunks}
    device_s = {name: parts[name]["median"] * 1e-6 * calls[name] for name in parts}
    return {"workload": f"C5 plan through the surface fitted on {fit.count} solved geometries (T = {fit.basis.n_terms}, N = {n}): {total} virtual geometries in chunks "
                        f"of {chunk}, three quantiles, limits at 3 sigma, screen",
            "fit": {"used": fit.count, "r2_min": float(np.nanmin(fit.r2)), "q2_min": float(np.nanmin(check.q2)), "loo_rms_max": float(np.nanmax(check.loo_rms)),
                    "max_leverage": check.max_leverage, "mean_leverage": check.mean_leverage},
            "validate_surface_ms": validate_ms, "virtual_wall_s": wall, "virtual_geometries_per_s": total / wall, "select_rounds": rounds, "chunks": chunks,
            "drawn": run.drawn, "dropped": run.dropped, "invalid": run.invalid, "joint_yield": run.screen.joint_yield,
            "per_chunk_us": parts, "calls": calls, "device_seconds_at_those_calls": device_s,
            "share_of_wall": {name: device_s[name] / wall for name in device_s},
            "hardpoint_table_bytes_per_chunk": int(sample.hardpoints.numel() * 8), "device_bytes_held": int(sample.hardpoints.numel() * 8 + sample.latents.numel() * 8 + out.numel() * 8 + 2 * rows)}


def measure(args) -> dict:
    import torch

    dp, plan, rel, columns = build(4096, args.steps_per_geometry, torch.device("cuda:0"))
    result = {"shapes": measure_shapes(args, dp, plan)}
    if int(args.virtual_geometries) > 0:
        result["virtual"] = measure_virtual(args, dp, plan, rel, columns)
    return result


def summary(result: dict) -> str:
    lines = []
    for r in result["shapes"]:
        f, t = r["fused_us"], r["torch_route_us"]
        lines.append(r["workload"])
        lines.append(f"    fused {f['median']:10.1f} us (interquartile {f['interquartile']:.1f})   basis + matmul + shift + where {t['median']:10.1f} us (interquartile "
                     f"{t['interquartile']:.1f})   fused / torch {r['fused_over_torch']:.2f}   faster by more than the margin ({r['margin_us']:.1f} us): "
                     f"{r['fused_faster_by_more_than_the_margin']}")
        lines.append(f"    {r['useful_fp64_flop_per_s'] / 1e12:.2f} TFLOP/s useful   peak above held: fused {r['peak_bytes_above_held']['fused'] / 1e6:.1f} MB, torch "
                     f"{r['peak_bytes_above_held']['torch'] / 1e6:.1f} MB (Phi {r['phi_table_bytes'] / 1e6:.1f} MB)   tables agree to "
                     f"{r['largest_gap_relative_to_the_largest_value']:.1e} of the largest value")
    v = result.get("virtual")
    if v:
        lines.append(v["workload"])
        lines.append(f"    fit: r2 from {v['fit']['r2_min']:.6f}, q2 from {v['fit']['q2_min']:.6f}, leverage max {v['fit']['max_leverage']:.3f} mean {v['fit']['mean_leverage']:.4f};"
                     f"   validate_surface {v['validate_surface_ms']:.2f} ms")
        lines.append(f"    virtual ensemble: {v['virtual_wall_s']:.2f} s wall = {v['virtual_geometries_per_s'] / 1e6:.2f} M geometries / s ({v['select_rounds']} select rounds x "
                     f"{v['chunks']} chunks); dropped {v['dropped']}, invalid {v['invalid']}, joint yield {v['joint_yield']:.6f}")
        for name, runs in v["per_chunk_us"].items():
            lines.append(f"    {name:13s}{runs['median']:10.1f} us per chunk (interquartile {runs['interquartile']:.1f}) x {v['calls'][name]:6d} calls = "
                         f"{v['device_seconds_at_those_calls'][name]:7.3f} s = {v['share_of_wall'][name]:.3f} of the wall time")
        lines.append(f"    the hardpoint table the virtual draw ignores: {v['hardpoint_table_bytes_per_chunk'] / 1e6:.1f} MB per chunk; device memory held "
                     f"{v['device_bytes_held'] / 1e6:.1f} MB whatever the ensemble's size")
    return "\n".join(lines) + "\n"


def main() -> int:
    ap = common.parser(rehearsal=False, steps_per_geometry=256, reps=20, virtual_geometries=1 << 24, chunk=65536)
    ap.add_argument("--geometries", default="4096,131072", help="the table sizes of (a)")
    return common.run(ap.parse_args(), measure, summary, echo=False)


if __name__ == "__main__":
    sys.exit(main())
