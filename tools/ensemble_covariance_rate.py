"""
What the on-device covariance pass costs (okx_ensemble_covariance, ShardedEnsemble(reduce=True, covariance=...)) on BASELINE
config 5 - 4096 perturbed geometries x 256 bump steps, bench.py's four metric columns: 1024 entries, a 32 MB table - on ONE
GPU, device events, 20 repetitions after warm-up, medians with the interquartile range:

  (a) the pass (used + partial Gram + merge) at N = 1024 - every entry - and at a 36-entry subset (4 columns x 9 evenly
      spaced steps);
  (b) in the same run, the torch formulation on the device: mask, shift, gather, fp64 d^T d;
  (c) what the user must otherwise do: metric_local.cpu() (timed alone), then ensemble_stats.covariance_host;
  (d) the ShardedEnsemble step with and without covariance= (the 36-entry subset), alternated.

The requirement: (a) at N = 1024 is faster than the copy ALONE of (c) measured in the same run.  The ratios to (b) and the
share of the fp64 peak are recorded, not required.

  python tools/ensemble_covariance_rate.py --out profiles/r11/ensemble_covariance_rate.json

``--rehearse N``: N ranks on cuda:0 over gloo (fresh child processes, each under the time limit), each writing its merged
accumulator to ``<out>/rank<r>.pt`` - the rehearsal tests/test_gpu_ensemble_covariance.py compares; ``--entries a,b,c`` selects
entries (default: all).
"""

from __future__ import annotations

import os
import statistics
import sys
import time

import ensemble_rate_common as common
from ensemble_rate_common import alternated, rank, spread, step_ms
from ensemble_reduce_rate import FP64_VECTOR_PEAK, HBM_PEAK, build


def subset(steps: int, n_columns: int, n_steps: int = 9) -> list:
    """Every column at ``n_steps`` evenly spaced steps (the first and the last among them)."""
    picks = sorted({round(i * (steps - 1) / max(1, n_steps - 1)) for i in range(n_steps)})
    return [s * n_columns + k for s in picks for k in range(n_columns)]


def rank_main(args) -> None:
    import torch

    from open_kinematics_amd.dist import ShardedEnsemble

    with rank(args) as device:
        dp, table, rel, columns = build(args.geometries, args.steps_per_geometry, device)
        entries = [int(x) for x in args.entries.split(",")] if args.entries else True
        pipe = ShardedEnsemble(dp, table, rel, args.steps_per_geometry, chunks=args.chunks or None, metric_columns=columns, reduce=True,
                               covariance=entries, chain_len=1, predictor=False)
        acc = pipe.step()
        torch.cuda.synchronize()
        merged, fin = pipe.covariance_accumulator, pipe.covariance()
        torch.save({"gram": merged.gram.cpu(), "sum": merged.sum.cpu(), "counts": merged.counts.cpu(), "entries": merged.entries.cpu(),
                    "shift": acc.shift.cpu(), "covariance": fin.covariance, "count": fin.count, "used": pipe.covariance_local_used.cpu(),
                    "sent": pipe.covariance_exchange_bytes_per_rank, "range": pipe.geometry_range, "pieces": pipe.pieces},
                   os.path.join(args.out, f"rank{args.rank}.pt"))


def rehearse(args) -> int:
    return common.rehearse(args, __file__, 38900, ["--geometries", args.geometries, "--steps-per-geometry", args.steps_per_geometry,
                                                        "--chunks", args.chunks, "--entries", args.entries], span=1000)


def measure(args) -> dict:
    import numpy as np
    import torch

    from open_kinematics_amd.dist import ShardedEnsemble
    from open_kinematics_amd.ensemble_stats import covariance_host

    device = torch.device("cuda:0")
    g, s = args.geometries, args.steps_per_geometry
    dp, table, rel, columns = build(g, s, device)
    k = len(columns)
    kw = dict(chain_len=1, predictor=False)
    few = subset(s, k)
    reduced = ShardedEnsemble(dp, table, rel, s, metric_columns=columns, reduce=True, **kw)
    covaried = ShardedEnsemble(dp, table, rel, s, metric_columns=columns, reduce=True, covariance=few, **kw)
    for _ in range(args.warmup):
        reduced.step()
        covaried.step()
    torch.cuda.synchronize()
    values, status, shift = covaried.metric_local, covaried.info_local[:, 32], covaried.local_accumulator.shift
    reps = args.reps

    # (a) the pass, (b) the torch formulation beside it - alternated block by block so that a drift hits all alike
    full = dp.covariance_ensemble(values, steps_per_geometry=s, status=status, shift=shift)
    part = dp.covariance_ensemble(values, steps_per_geometry=s, status=status, shift=shift, entries=few)
    index = torch.as_tensor(few, device=device, dtype=torch.int64)

    def torch_form(at):
        def run():
            v = values.view(g, s * k)
            ok = (torch.isfinite(v) & ((status & 7) == 1).view(g, s, 1).expand(g, s, k).reshape(g, s * k))
            sh = shift.reshape(-1)
            if at is not None:
                v, ok, sh = v.index_select(1, at), ok.index_select(1, at), sh.index_select(0, at)
            used = ok.all(dim=1, keepdim=True)
            d = torch.where(used, v - sh, torch.zeros((), dtype=torch.float64, device=device))
            return d.t() @ d, d.sum(dim=0), used.sum()
        return run

    other = dp.covariance_ensemble(values, steps_per_geometry=s, status=status, shift=shift)

    def valu_pass():  # the register-tiled v_fma_f64 form of the partial Gram kernel (a developer switch, read per launch)
        os.environ["OKX_DEV"] = "cov_valu"
        try:
            dp.covariance_ensemble(values, steps_per_geometry=s, status=status, out=other)
        finally:
            del os.environ["OKX_DEV"]

    fns = {"pass_1024": lambda: dp.covariance_ensemble(values, steps_per_geometry=s, status=status, out=full), "pass_1024_valu": valu_pass,
           "pass_36": lambda: dp.covariance_ensemble(values, steps_per_geometry=s, status=status, out=part),
           "torch_1024": torch_form(None), "torch_36": torch_form(index)}
    runs = alternated(fns, reps)
    med = {name: statistics.median(r) for name, r in runs.items()}
    valu_gap = float(((full.gram - other.gram).abs() / torch.sqrt(torch.outer(torch.diag(full.gram), torch.diag(full.gram))).clamp_min(1e-300)).max())
    t_gram, t_sum, t_used = torch_form(None)()
    torch.cuda.synchronize()
    scale = torch.sqrt(torch.outer(torch.diag(full.gram), torch.diag(full.gram)))
    torch_gap = float(((full.gram - t_gram).abs() / torch.where(scale > 0, scale, torch.ones_like(scale))).max())

    # (c) what the user must otherwise do on one GPU
    copy_ms, host_ms = [], []
    for rep in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = values.cpu()  # the copy alone: the table, without its status bytes
        t1 = time.perf_counter()
        copy_ms.append((t1 - t0) * 1e3)
        if rep >= 1:  # (the NumPy part is not what the comparison is about: one run of it, on the subset)
            continue
        want = covariance_host(host.numpy().reshape(g, s, k), status.cpu().numpy().reshape(g, s), few, shift.cpu().numpy())
        host_ms.append((time.perf_counter() - t1) * 1e3)
    got = part.numpy()
    d = np.abs(np.where(want.used[:, None].astype(bool), host.numpy().reshape(g, s * k)[:, few] - shift.cpu().numpy().reshape(-1)[few][None], 0.0))
    within = bool(np.all(np.abs(got.gram - want.gram) <= 2 * (g + 2) * 2.0 ** -53 * (d.T @ d) * (1 + 1e-9)) and np.array_equal(got.counts, want.counts)
                  and np.array_equal(got.used, want.used))

    # (d) the sharded ensemble's step with and without the covariance, alternated
    rounds = [(step_ms(reduced.step, args.steps), step_ms(covaried.step, args.steps)) for _ in range(5)]
    off, on = statistics.median(r[0] for r in rounds), statistics.median(r[1] for r in rounds)

    one = lambda name: {"median": med[name], "interquartile": spread(runs[name]), "runs": runs[name]}  # noqa: E731
    n = s * k
    flop = float(n) * (n + 1) * g  # the lower triangle with its diagonal: one multiply and one add per product
    table_bytes = 8 * g * s * k + g * s
    copy = statistics.median(copy_ms)
    return {
        "workload": f"C5: {g} geometries x {s} steps, {k} metric columns: {n} entries, one GPU",
        "inner_product": {"shipped": "v_mfma_f64_16x16x4_f64, 2 x 2 accumulators per wavefront", "mfma_us": med["pass_1024"],
                          "valu_4x4_register_tile_us": one("pass_1024_valu"), "valu_over_mfma": med["pass_1024_valu"] / med["pass_1024"],
                          "largest_gap_between_the_two_in_units_of_the_diagonal": valu_gap},
        "used_dropped": [int(x) for x in full.counts.cpu()],
        "a_pass_us": {"n_1024": {**one("pass_1024"), "lower_triangle_flop": flop, "tflops": flop / med["pass_1024"] * 1e-6,
                                 "share_of_fp64_peak": flop / med["pass_1024"] * 1e6 / FP64_VECTOR_PEAK, "table_bytes": table_bytes,
                                 "hbm_floor_us": table_bytes / HBM_PEAK * 1e6,
                                 "scratch_bytes": int(dp.lib.okx_ensemble_covariance_scratch_bytes(g, s, k, n))},
                      "n_36": {**one("pass_36"), "entries": few}},
        "b_torch_on_device_us": {"n_1024": one("torch_1024"), "n_36": one("torch_36"), "pass_over_torch_1024": med["pass_1024"] / med["torch_1024"],
                                 "pass_over_torch_36": med["pass_36"] / med["torch_36"], "largest_gap_to_torch_in_units_of_the_diagonal": torch_gap,
                                 "torch_counts_agree": bool(int(t_used) == int(full.counts[0]))},
        "c_host_path_ms": {"copy_alone_median": copy, "copy_interquartile": spread(copy_ms), "copy_runs": copy_ms,
                           "numpy_covariance_36_entries": statistics.median(host_ms),
                           "what": "metric_local.cpu() alone; then the status bytes' copy and ensemble_stats.covariance_host on the 36 entries"},
        "requirement_pass_1024_faster_than_the_copy_alone": {"pass_us": med["pass_1024"], "copy_us": copy * 1e3, "holds": bool(med["pass_1024"] < copy * 1e3)},
        "device_within_bound_of_covariance_host_36": within,
        "d_step_ms": {"reduce_only": off, "with_covariance_36": on, "extra_ms": on - off, "extra_percent": (on / off - 1.0) * 100.0, "rounds": rounds,
                      "steps_per_round": args.steps},
        "covariance_exchange_bytes_per_rank": {"n_36": 8 * (36 * 36 + 36 + 2), "n_1024": 8 * (n * n + n + 2)},
    }


def summary(r: dict) -> str:
    a, b, c, d, e = r["a_pass_us"], r["b_torch_on_device_us"], r["c_host_path_ms"], r["d_step_ms"], r["requirement_pass_1024_faster_than_the_copy_alone"]
    big, few = a["n_1024"], a["n_36"]
    ip = r["inner_product"]
    lines = [r["workload"], f"geometries used, dropped: {r['used_dropped']}",
             f"inner product: {ip['shipped']}: {ip['mfma_us']:.1f} us; the v_fma_f64 4 x 4 register tile (OKX_DEV=cov_valu): "
             f"{ip['valu_4x4_register_tile_us']['median']:.1f} us (interquartile {ip['valu_4x4_register_tile_us']['interquartile']:.1f}), {ip['valu_over_mfma']:.2f} x",
             f"(a) pass, N = 1024       {big['median']:9.1f} us  (interquartile {big['interquartile']:.1f}; {big['tflops']:.2f} TFLOP/s on the lower triangle, "
             f"{big['share_of_fp64_peak'] * 100:.1f} % of the fp64 peak; the table's bytes at the HBM peak: {big['hbm_floor_us']:.1f} us)",
             f"    pass, N = 36         {few['median']:9.1f} us  (interquartile {few['interquartile']:.1f})",
             f"(b) torch, N = 1024      {b['n_1024']['median']:9.1f} us  (interquartile {b['n_1024']['interquartile']:.1f})   pass / torch = {b['pass_over_torch_1024']:.2f}",
             f"    torch, N = 36        {b['n_36']['median']:9.1f} us  (interquartile {b['n_36']['interquartile']:.1f})   pass / torch = {b['pass_over_torch_36']:.2f}",
             f"(c) copy alone           {c['copy_alone_median'] * 1e3:9.1f} us  (interquartile {c['copy_interquartile'] * 1e3:.1f})   NumPy covariance, 36 entries: "
             f"{c['numpy_covariance_36_entries']:.1f} ms",
             "    requirement, the pass at N = 1024 faster than the copy alone: " + ("holds" if e["holds"] else "MISSED")
             + f" ({e['pass_us']:.1f} us against {e['copy_us']:.1f} us)",
             f"    device within the summation bound of covariance_host (36 entries), counts and used bytes equal: {r['device_within_bound_of_covariance_host_36']}",
             f"(d) step                 {d['reduce_only']:.3f} ms reduce only, {d['with_covariance_36']:.3f} ms with covariance of 36 entries "
             f"(+{d['extra_ms']:.3f} ms, {d['extra_percent']:.1f} %)"]
    return "\n".join(lines) + "\n"


def main() -> int:
    ap = common.parser(geometries=4096, steps_per_geometry=256, steps=50, warmup=10, reps=20, chunks=0)
    ap.add_argument("--entries", default="")
    return common.run(ap.parse_args(), measure, summary, rank_main, rehearse)


if __name__ == "__main__":
    sys.exit(main())
