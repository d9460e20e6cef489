"""
What the response-surface passes cost (okx_ensemble_basis, okx_ensemble_surface) on BASELINE config 5's shape - geometries of the perturbed
double wishbone drawn by the sampler (LHS, 30 latents) x 256 bump steps, bench.py's four metric columns - for P = 10 and 30 latents (degree 2
with interactions: T = 66 and 496 terms) and N = 36 and all 1024 entries, at 4096 geometries (C5) and at 131 072, on ONE GPU, device events,
20 repetitions after warm-up, alternated block by block so that a drift hits every pass alike:

  (a) the basis pass (once per ensemble: factors do not change from step to step);
  (b) the surface pass, beside okx_ensemble_covariance of the same N entries and okx_ensemble_reduce (no factors) over the same table; its
      useful fp64 rate - G (T (T + 1) + 2 T N) operations, the lower triangle of Phi^T Phi and the rectangle Phi^T D - as a share of the
      78.6e12 the matrix units retire;
  (c) the torch route on the device: gather the entries, subtract, the complete-case vote, Phi.T @ Phi and Phi.T @ D - the mask and valid
      votes, which do not change from step to step, are made once outside the timed region (it materialises D and a masked Phi and gives no fixed bits);
  (d) the host route: the table's .cpu() (timed alone), then the gathered entries and numpy.linalg.lstsq - timed on the first
      --host-geometries geometries only (it is linear in them) and scaled.

Nobody had measured this pass; no target is fixed, but the pass must beat the host route.  The device accumulator of the first geometries is
compared with surface_host's: counts equal, the sums within 2 (n + 1) u sum |term|.

  python tools/ensemble_surface_rate.py --out profiles/r25/ensemble_surface_rate.json

``--rehearse N``: N ranks on one GPU over gloo (fresh child processes) run ``ShardedEnsemble(reduce=True, factors="sampled", surface=True)`` over
``--geometries`` geometries of a plan over the first ``--points`` points, each saving its merged accumulator (tests/test_gpu_ensemble_surface.py).
"""

from __future__ import annotations

import os
import statistics
import sys
import time

import ensemble_rate_common as common
from ensemble_effects_rate import build
from ensemble_rate_common import timed

U = 2.0 ** -53
FP64_MATRIX_PEAK = 78.6e12


def rank_main(args) -> None:
    import torch

    from open_kinematics_amd.dist import ShardedEnsemble

    with common.rank(args) as device:
        dp, plan, rel, columns = build(int(args.geometries), args.steps_per_geometry, device, n_points=args.points or None)
        pipe = ShardedEnsemble(dp, plan, rel, args.steps_per_geometry, chunks=args.chunks or None, metric_columns=columns, reduce=True, factors="sampled",
                               surface=True, chain_len=1, predictor=False)
        acc = pipe.step()
        torch.cuda.synchronize()
        merged = pipe.surface_accumulator
        torch.save({"gram": merged.gram.cpu(), "cross": merged.cross.cpu(), "sumsq": merged.sumsq.cpu(), "counts": merged.counts.cpu(),
                    "entries": merged.entries.cpu(), "shift": acc.shift.cpu(), "coefficients": pipe.surface().coefficients,
                    "used": pipe.stages["surface"].local.used.cpu(), "sent": pipe.surface_exchange_bytes_per_rank, "range": pipe.geometry_range,
                    "pieces": pipe.pieces}, os.path.join(args.out, f"rank{args.rank}.pt"))


def rehearse(args) -> int:
    return common.rehearse(args, __file__, 41900, ["--geometries", args.geometries, "--steps-per-geometry", args.steps_per_geometry, "--chunks", args.chunks,
                                                        "--points", args.points], span=1000)


def measure_one(args, n_geom: int) -> list:
    import numpy as np
    import torch

    from open_kinematics_amd.dist import ShardedEnsemble
    from open_kinematics_amd.ensemble_stats import basis_host, surface_host, surface_terms

    device = torch.device("cuda:0")
    s, reps = args.steps_per_geometry, args.reps
    dp, plan, rel, columns = build(n_geom, s, device)
    k = len(columns)
    few_entries = [step * k + c for step in np.linspace(0, s - 1, 9).astype(int) for c in range(k)]  # 36 entries: nine steps of the sweep
    pipe = ShardedEnsemble(dp, plan, rel, s, metric_columns=columns, reduce=True, factors="sampled", surface=dict(factors=list(range(10)), entries=few_entries),
                           chain_len=1, predictor=False)
    t0 = time.perf_counter()
    pipe.step()
    torch.cuda.synchronize()
    first_step_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    pipe.step()
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t0) * 1e3
    fit = pipe.surface()
    mid = 4 * k  # camber at mid sweep
    chain = {"step_ms": {"first": first_step_ms, "second": step_ms}, "used": fit.count, "camber_at_mid_sweep": {
        "r2": float(fit.r2[mid]), "largest_first": float(np.nanmax(fit.first[:, mid])), "largest_interaction": float(np.nanmax(fit.interaction[:, :, mid])),
        "sum_of_interactions": float(np.nansum(fit.interaction[:, :, mid]) / 2.0)}}
    table, status, flags, latents = pipe.metric_local, pipe.info_local[:, 32], pipe.sampled_flags, pipe.my_factors
    shift = pipe.local_accumulator.shift
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
    for p in (10, 30):
        basis = surface_terms(plan, factors=list(range(p)))
        t = basis.n_terms
        rows = dp.basis_factors(latents, basis)
        for entries in (few_entries, None):
            n = s * k if entries is None else len(entries)
            acc = dp.surface_ensemble(table, steps_per_geometry=s, basis_table=rows, status=status, mask=flags, entries=entries, shift=shift)
            cacc = dp.covariance_ensemble(table, steps_per_geometry=s, status=status, entries=entries, shift=shift)
            index = torch.arange(n, device=device) if entries is None else torch.as_tensor(entries, device=device)
            flat_shift = shift.reshape(-1)[index]

            open_rows = ((flags & 1) == 0) & (rows.valid != 0)  # (made once: neither the mask nor the basis rows change from step to step)
            step_of = index // k

            def torch_route():
                d = table.reshape(n_geom, s * k)[:, index] - flat_shift
                okay = (status.reshape(n_geom, s) & 7) == 1
                used = torch.isfinite(d).all(dim=1) & okay[:, step_of].all(dim=1) & open_rows
                d = torch.where(used[:, None], d, torch.zeros_like(d))
                f = rows.phi * used[:, None]
                return f.t() @ f, f.t() @ d, (d * d).sum(dim=0), used.sum()

            runs = timed(reps=reps, passes={"basis": lambda: dp.basis_factors(latents, out=rows),
                                            "surface": lambda: dp.surface_ensemble(table, steps_per_geometry=s, basis_table=rows, status=status, mask=flags, out=acc),
                                            "covariance": lambda: dp.covariance_ensemble(table, steps_per_geometry=s, status=status, out=cacc),
                                            "reduce": lambda: dp.reduce_ensemble(table, steps_per_geometry=s, status=status, out=racc),
                                            "torch": torch_route})
            torch.cuda.synchronize()
            tg, tc, tq, tu = (x.cpu().numpy() for x in torch_route())
            whole = acc.numpy()
            # the host route on the first geometries
            t0 = time.perf_counter()
            phi, valid = basis_host(lat, basis)
            at = np.arange(s * k) if entries is None else np.asarray(entries)
            cols = values.reshape(few, s * k)[:, at]
            ok = np.isfinite(cols).all(axis=1) & np.repeat((st & 7) == 1, k, axis=1)[:, at].all(axis=1) & ((fl & 1) == 0) & (valid != 0)
            d = cols[ok] - sh.reshape(-1)[at]
            coefficients, *_ = np.linalg.lstsq(phi[ok], d, rcond=None)
            host_ms = (time.perf_counter() - t0) * 1e3
            check = None
            if t * n <= 66 * 1024:  # (surface_host walks the geometries one by one: the definition is compared where that is quick)
                want = surface_host(values, st, fl, phi, valid, entries, sh, basis=basis)
                got = dp.surface_ensemble(table[: few * s], steps_per_geometry=s, basis_table=dp.basis_factors(latents[:few], basis), status=status[: few * s],
                                          mask=flags[:few], entries=entries, shift=shift).numpy()
                c = 2.0 * (few + 1) * U
                f, a = np.abs(np.where(ok[:, None], phi, 0.0)), np.abs(np.where(ok[:, None], cols - sh.reshape(-1)[at], 0.0))
                ratios = [np.max(np.abs(got.gram - want.gram) / np.maximum(c * (f.T @ f), 1e-300)), np.max(np.abs(got.cross - want.cross) / np.maximum(c * (f.T @ a), 1e-300)),
                          np.max(np.abs(got.sumsq - want.sumsq) / np.maximum(c * (a * a).sum(axis=0), 1e-300))]
                fitted = got.finalize().coefficients
                check = {"counts_equal_surface_host": bool(np.array_equal(got.counts, want.counts)), "largest_difference_over_bound": float(max(ratios)),
                         "coefficients_against_lstsq_relative": float(np.max(np.abs(fitted - coefficients) / np.abs(coefficients).max(axis=0)))}
            seconds = runs["surface"]["median"] * 1e-6
            flop = n_geom * (t * (t + 1) + 2.0 * t * n)
            scale = np.maximum(np.abs(whole.gram), 1.0)
            out.append({
                "workload": f"C5 sampled (LHS): {n_geom} geometries x {s} steps, {k} metric columns, P = {p} latents, T = {t} terms, N = {n} entries, one GPU",
                "a_basis_us": runs["basis"], "b_surface_us": runs["surface"], "b_covariance_us": runs["covariance"], "b_reduce_us": runs["reduce"],
                "c_torch_route_us": runs["torch"],
                "surface_over_covariance": runs["surface"]["median"] / runs["covariance"]["median"],
                "surface_over_torch": runs["surface"]["median"] / runs["torch"]["median"],
                "useful_fp64_flop_per_s": flop / seconds, "share_of_matrix_peak": flop / seconds / FP64_MATRIX_PEAK,
                "phi_table_bytes": 8 * n_geom * t, "scratch_bytes": int(dp.lib.okx_ensemble_surface_scratch_bytes(n_geom, s, k, t, n)),
                "used": int(whole.counts[0]), "torch_route_used_equal": bool(int(tu) == int(whole.counts[0])),
                "torch_route_gram_relative_gap": float(np.max(np.abs(tg - whole.gram) / scale)),
                "d_host_path_ms": {"copy_alone_median": statistics.median(copy_ms), "copy_runs": copy_ms, "host_geometries": few,
                                   "basis_host_gather_and_lstsq": host_ms, "scaled_to_the_table": host_ms * n_geom / few},
                "device_pass_ms_basis_plus_surface": (runs["basis"]["median"] + runs["surface"]["median"]) * 1e-3,
                "check": check, "chain": chain if p == 10 and entries is not None else None,
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
        a, b, cv, rd, tr, h = r["a_basis_us"], r["b_surface_us"], r["b_covariance_us"], r["b_reduce_us"], r["c_torch_route_us"], r["d_host_path_ms"]
        lines.append(r["workload"])
        lines.append(f"(a) basis   {a['median']:10.1f} us (interquartile {a['interquartile']:.1f})   Phi {r['phi_table_bytes'] / 1e6:.1f} MB")
        lines.append(f"(b) surface {b['median']:10.1f} us (interquartile {b['interquartile']:.1f})   covariance, same entries {cv['median']:9.1f} us (ratio "
                     f"{r['surface_over_covariance']:.2f})   reduce {rd['median']:9.1f} us   {r['useful_fp64_flop_per_s'] / 1e12:.2f} TFLOP/s useful = "
                     f"{r['share_of_matrix_peak']:.3f} of the fp64 matrix peak   scratch {r['scratch_bytes'] / 1e6:.1f} MB")
        lines.append(f"(c) torch route {tr['median']:10.1f} us (interquartile {tr['interquartile']:.1f})   surface / torch {r['surface_over_torch']:.2f}   used equal: "
                     f"{r['torch_route_used_equal']}, gram gap {r['torch_route_gram_relative_gap']:.2e} relative")
        lines.append(f"(d) host route: copy alone {h['copy_alone_median']:.1f} ms, then basis_host + gather + lstsq {h['scaled_to_the_table']:.0f} ms (timed on "
                     f"{h['host_geometries']} geometries: {h['basis_host_gather_and_lstsq']:.0f} ms);   device basis + surface {r['device_pass_ms_basis_plus_surface']:.3f} ms")
        if r["check"]:
            c = r["check"]
            lines.append(f"    against surface_host: counts equal {c['counts_equal_surface_host']}, largest difference {c['largest_difference_over_bound']:.3f} of "
                         f"2 (n + 1) u sum |term|; coefficients against lstsq {c['coefficients_against_lstsq_relative']:.2e} relative")
        if r["chain"]:
            c = r["chain"]
            m = c["camber_at_mid_sweep"]
            lines.append(f"    chain step (rebind, evaluated solve, reduce, basis once, surface): {c['step_ms']['second']:.1f} ms; camber at mid sweep: r2 {m['r2']:.4f}, "
                         f"largest first-order share {m['largest_first']:.3f}, largest pairwise share {m['largest_interaction']:.2e}, all pairs {m['sum_of_interactions']:.2e}")
    return "\n".join(lines) + "\n"


def main() -> int:
    ap = common.parser(steps_per_geometry=256, reps=20, host_geometries=4096, chunks=0, points=0)
    ap.add_argument("--geometries", default="4096,131072", help="the ensemble sizes to measure (a rehearsal: one size)")
    return common.run(ap.parse_args(), measure, summary, rank_main, rehearse, echo=False)


if __name__ == "__main__":
    sys.exit(main())
